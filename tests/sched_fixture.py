"""The input and the reference golden of the schedule tests (test_golden_sched.py, test_gpu_schedule.py).

One sweep small enough to rerun after every edit that still takes the engine's MFMA path under every stop rule
(m_pad = 1152 > 1024, n = 72 > 64): A = planted_matrix(1100, 72), k = 2..10, R = 12, seed 123: 108 jobs, 648 stacked
columns, 11 live panels in the first packing.  tests/golden/golden_sched.npz holds what the reference's own nmf_mu gives
for each job (tests/golden/make_golden_sched.py); A is regenerated here and pinned by its SHA-256.
"""
import functools
import hashlib
import os

import numpy as np

GOLDEN_SCHED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_sched.npz")
M, N, KS, R, SEED, MAXITER = 1100, 72, list(range(2, 11)), 12, 123, 10000
NJ = len(KS) * R


@functools.lru_cache(maxsize=None)
def golden_sched():
    with np.load(GOLDEN_SCHED, allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    for v in g.values():
        v.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def sched_A():
    from nmfconsensus_amd.synthetic import planted_matrix
    A = planted_matrix(M, N)
    A.setflags(write=False)
    return A


def sha256_of(A) -> str:
    return hashlib.sha256(np.asfortranarray(A).tobytes(order="F")).hexdigest()
