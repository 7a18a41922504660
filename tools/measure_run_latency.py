#!/usr/bin/env python3
"""Wall time of the one-shot drop-in call qgemul_run (host buffers in, host buffers out) for small and large problems, and of the
batched and the grouped one-shot call on three small members.  Needs an MI355X."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qublas_amd import capi  # noqa: E402
from qublas_amd.desc import Qu, SAT, TRN, Tags, lower  # noqa: E402

E88 = Qu(8, 8, True, TRN.TCPL, SAT.ZERO)
rng = np.random.default_rng(1)
for S, kw, reps in ((4, dict(mul_args=E88, add_args=[E88]), 200), (64, dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)]), 200),
                    (512, dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)]), 50), (4096, dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)]), 5)):
    ec = E88 if S == 4 else Qu(23, 8)
    d = lower(E88, E88, ec, S, S, S, **kw)
    A = rng.integers(E88.raw_min, E88.raw_max + 1, S * S, dtype=np.int32)
    B = rng.integers(E88.raw_min, E88.raw_max + 1, S * S, dtype=np.int32)
    C = np.zeros(S * S, dtype=np.int32)
    capi.run(d, C, A, B)
    t0 = time.perf_counter()
    for _ in range(reps):
        capi.run(d, C, A, B)
    dt = (time.perf_counter() - t0) / reps
    print(json.dumps({"S": S, "kernel": capi.KERNEL_NAMES[capi.classify(d).kernel], "ms_per_call": dt * 1e3}), flush=True)

# the batched and the grouped one-shot call on small members: int<7,8> operands, two limbs each, every member in the one launch
Q78 = Qu(7, 8)
GROUP = [(65, 33, 100), (3, 5, 7), (33, 17, 64)]
descs = [lower(Q78, Q78, Qu(20, 8), M, N, K, mul_args=Tags(15, 16), add_args=[Qu(28, 16)]) for M, N, K in GROUP]
As = [rng.integers(Q78.raw_min, Q78.raw_max + 1, M * K, dtype=np.int32) for M, N, K in GROUP]
Bs = [rng.integers(Q78.raw_min, Q78.raw_max + 1, K * N, dtype=np.int32) for M, N, K in GROUP]
Cs = [np.zeros(M * N, dtype=np.int32) for M, N, K in GROUP]
M, N, K = GROUP[0]
A3, B3, C3 = np.concatenate([As[0]] * 3), np.concatenate([Bs[0]] * 3), np.zeros(3 * M * N, dtype=np.int32)
calls = (("batched 3 x (65,33,100)", capi.classify_batched_status(descs[0], 3)[1], lambda: capi.run_batched(descs[0], 3, C3, A3, B3, M * N, M * K, K * N)),
         ("grouped (65,33,100) (3,5,7) (33,17,64)", capi.classify_grouped_status(descs)[1], lambda: capi.run_grouped(descs, Cs, As, Bs)))
for name, info, call in calls:
    call()
    t0 = time.perf_counter()
    for _ in range(200):
        call()
    dt = (time.perf_counter() - t0) / 200
    print(json.dumps({"call": name, "kernel": capi.KERNEL_NAMES[info.kernel], "ms_per_call": dt * 1e3}), flush=True)
