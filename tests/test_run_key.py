"""The one-shot calls' plan key (qublas_amd/csrc/qg_run_key.h: QRunKey, qg_run_key_set, qg_run_key_equal) under AddressSanitizer +
UndefinedBehaviorSanitizer on the CPU.  The header has no HIP types, so the host compiler builds tests/san/run_key_driver.cpp with it
alone.  For one descriptor and one group of three the driver builds the key of every kind of request (plain, real chain, with one
APPROX table and with another, complex chain, with a CMUL record and with another, batched at one, two and seven members, batched
chain with a stage shared and per member; a group of one, of three, the three with only the last member's K changed and in another
order, a grouped chain without and with a scalar stage per member, and the batched chain of the same count whose shared flags have
that same bit pattern) and checks that
  (a) a key equals the key built from copies of its inputs whose padding, reserved bytes and unused entries differ — the entries
      of a group's descriptor list included,
  (b) two different kinds never compare equal, in either order (a group of one, the plain request and a batch of one among them),
  (c) a key set (or assigned) over one that held a larger request — the largest batched chain, and the grouped chain — equals a
      freshly built one: a plain key over a grouped one drops the list, a group of one over a group of three shortens it.
Leak detection is on: the key owns its APPROX tables and its descriptor list."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_run_key_under_asan_ubsan(tmp_path):
    exe = os.path.join(str(tmp_path), "run_key_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "san", "run_key_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout.decode()[-3000:], r.stderr.decode()[-3000:])
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr.decode()[-3000:]
    assert r.stdout.decode().startswith("ok "), r.stdout.decode()[-3000:]
