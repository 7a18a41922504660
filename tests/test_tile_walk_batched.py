"""The block-diagonal walk of the batched Qgemul (qg_bd_tile_of in qublas_amd/csrc/qg_tile_walk.h) on the CPU: the host compiler builds
the header with -fsanitize=address,undefined (as tests/test_tile_walk.py does) and this test compares what it prints, for every
workgroup of every swept batch, with a restatement: the workgroups map one to one onto (member, tile), and a member's tiles are
consecutive tile numbers, so that they sit in one XCD residue class's run of the walk (or straddle two neighbouring runs)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 2, 7, 8, 9, 300)
TILE_ROWS = (1, 2, 3, 8, 9, 10, 17)      # qg_tile_of<8, true> walks a member in groups of 8 tile rows: one group, exactly one, a ragged second and third
TILE_COLS = (1, 2, 3, 5)


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tile_walk_bd") / "tile_walk_bd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "san", "tile_walk_batched_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr.decode()[-3000:]
    out = {}
    for ln in r.stdout.decode().splitlines():
        kind, _, rest = ln.partition(" ")
        assert kind == "bd"
        key, _, vals = rest.partition(" :")
        v = [int(x) for x in vals.split()]
        out[tuple(int(x) for x in key.split())] = list(zip(v[0::3], v[1::3], v[2::3]))
    return out


def run_start(nwg, x):
    q, r = nwg // 8, nwg % 8
    return x * (q + 1) if x < r else r * (q + 1) + (x - r) * q


def tile_of(w, tiles_m, tiles_n, gm=8):
    grp = w // (gm * tiles_n)
    first_m = grp * gm
    gsz = min(tiles_m - first_m, gm)
    rem = w % (gm * tiles_n)
    return first_m + rem % gsz, rem // gsz


def bd_tile_of(w, tmM, tnN):
    """tile number of the batch -> (member, tile_m, tile_n): members one after the other, each walked as one GEMM is"""
    return (w // (tmM * tnN),) + tile_of(w % (tmM * tnN), tmM, tnN)


def test_every_workgroup_of_every_batch(printed):
    n = 0
    for tmM in TILE_ROWS:
        for tnN in TILE_COLS:
            for batch in BATCHES:
                nwg = batch * tmM * tnN
                got = printed[(tmM, tnN, batch)]
                assert len(got) == nwg
                exp = [bd_tile_of(run_start(nwg, bid % 8) + bid // 8, tmM, tnN) for bid in range(nwg)]
                assert got == exp, (tmM, tnN, batch)
                # a bijection onto (member, tile_m, tile_n)
                assert sorted(got) == [(b, m, c) for b in range(batch) for m in range(tmM) for c in range(tnN)], (tmM, tnN, batch)
                # member-contiguous: in the order of the walk (tile number w), the members come one after the other
                by_w = {run_start(nwg, bid % 8) + bid // 8: got[bid] for bid in range(nwg)}
                assert sorted(by_w) == list(range(nwg))
                assert [by_w[w][0] for w in range(nwg)] == [w // (tmM * tnN) for w in range(nwg)], (tmM, tnN, batch)
                n += 1
    assert n == len(TILE_ROWS) * len(TILE_COLS) * len(BATCHES)
