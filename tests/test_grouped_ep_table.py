"""The tile -> member table of a grouped chain's pass (qublas_amd/csrc/qg_grp.h: qg_grp_tile_members) on the CPU: the host compiler
builds the header with -fsanitize=address,undefined into a stand-alone program (tests/san/grouped_tile_member_driver.cpp, as
tests/test_grouped_schedule.py does) and this test compares what it prints, for swept groups, with a restatement.

The restated rule: the packed C of the launch holds the members in LIST order, each with tiles_m * tiles_n tiles of 64 x 64
elements; entry w of the table is the member (its index in the caller's list) whose tiles cover position w.  Against the schedule:
every record's c_off / 4096 is a position of the table, every position occurs in exactly one record, and the record's member is the
table's entry there."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TILE = 64 * 64


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grouped_tile_member") / "grouped_tile_member")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "san", "grouped_tile_member_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr.decode()[-3000:]
    return [json.loads(l) for l in r.stdout.decode().splitlines()]


def test_the_sweep_is_the_one_the_driver_documents(printed):
    assert len(printed) == 6 * 4
    assert sorted({len(g["members"]) for g in printed}) == [1, 2, 7, 8, 9, 300]
    assert {(tm, tn) for g in printed for tm, tn, _ in g["members"]} == {(0, 1), (1, 1), (2, 1), (3, 3), (9, 2), (17, 5)}
    assert any(len(g["table"]) >= 64 and len(g["table"]) % 64 for g in printed)          # dealt rounds and a ragged tail


def test_table_equals_the_restatement(printed):
    for g in printed:
        want = [member for tm, tn, member in g["members"] for _ in range(tm * tn)]
        assert g["table"] == want


def test_members_are_in_list_order_of_memory(printed):
    for g in printed:
        assert g["table"] == sorted(g["table"])                                           # (member numbers rise along the list)
        assert set(g["table"]) == {member for tm, tn, member in g["members"] if tm * tn}


def test_bijection_with_the_schedule(printed):
    for g in printed:
        T = len(g["table"])
        assert len(g["schedule"]) == T
        pos = [c_off // C_TILE for c_off, _ in g["schedule"]]
        assert all(c_off % C_TILE == 0 for c_off, _ in g["schedule"])
        assert sorted(pos) == list(range(T))                                              # every C tile in exactly one workgroup's record
        for (c_off, member), w in zip(g["schedule"], pos):
            assert g["table"][w] == member
