"""Every planner answer of a fixed, seeded sweep, one line per query: the acceptance check of a change that must not move a planner
decision (run it in the parent's checkout and in the branch's; the two outputs must be byte-identical).

    python tools/dump_geometry.py [--out FILE]        # prints (or writes) the dump, then "# N lines, sha256 H" on stderr

CPU only: it asks the loaded library's classify entry points (qublas_amd.capi).  The sweep is tests/geom_sweep.py at the size below:
at least 20 000 plain, 2 000 batched and 500 grouped queries.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="write the dump here instead of stdout")
    a = ap.parse_args()
    import geom_sweep as S
    qs = S.queries(n_random=2400, n_compact=800, n_groups=60)
    count = {"plain": 0, "batched": 0, "grouped": 0}
    lines = []
    for i, q in enumerate(qs):
        count[q[0]] += 1
        lines.append(f"{i} {q[0]} {json.dumps(S.ask_library(q), sort_keys=True)}")
    assert count["plain"] >= 20000 and count["batched"] >= 2000 and count["grouped"] >= 500, count
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    print(f"# {len(lines)} lines ({count['plain']} plain, {count['batched']} batched, {count['grouped']} grouped), sha256 {hashlib.sha256(text.encode()).hexdigest()}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
