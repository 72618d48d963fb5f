"""Fixture conditions of tests/golden/golden_sched.npz: what tests/test_gpu_schedule.py relies on.  No GPU."""
import numpy as np

from sched_fixture import KS, M, MAXITER, N, NJ, R, SEED, golden_sched, sched_A, sha256_of


def test_sched_golden_conditions():
    g = golden_sched()
    A = sched_A()
    assert A.shape == (M, N) == (int(g["m"]), int(g["n"]))
    assert sha256_of(A) == str(g["A_sha256"])   # the GPU tests regenerate the matrix the reference ran on
    assert [int(k) for k in g["ks"]] == KS and int(g["R"]) == R and int(g["seed"]) == SEED
    assert int(g["maxiter"]) == MAXITER
    assert np.array_equal(g["job_k"], np.array(KS * R, dtype=np.int32))   # expand.grid order, k fastest
    it = g["iters"]
    assert it.shape == (NJ,) and it.dtype == np.int32
    # every job exits by the stop rule, at many different iterations, with enough jobs on either side of the
    # maxiter = 451 cap the GPU tests run
    assert it.max() < MAXITER and it.min() > 0
    assert len(np.unique(it)) >= 30
    assert (it <= 450).sum() >= 20
    assert (it > 450).sum() >= 20
    # the stored factors: the shortest job, the longest, and the k = 10 job of median length
    hj = [int(j) for j in g["H_jobs"]]
    assert it[hj[0]] == it.min() and it[hj[1]] == it.max()
    k10 = np.where(g["job_k"] == 10)[0]
    assert hj[2] in k10 and it[hj[2]] == np.sort(it[k10])[len(k10) // 2]
    for q, j in enumerate(hj):
        H = g[f"H_{q}"]
        assert H.shape == (g["job_k"][j], N) and np.isfinite(H).all() and (H >= 0).all()
        assert np.array_equal(np.argmax(H, axis=0) + 1, g["labels_argmax"][j])
        assert np.array_equal(np.argmin(H, axis=0) + 1, g["labels_rorder"][j])
    # labels and counts under both rules are consistent with each other
    for key in ("argmax", "rorder"):
        L, C = g[f"labels_{key}"], g[f"counts_{key}"]
        assert L.shape == (NJ, N) and L.dtype == np.int32 and C.shape == (len(KS), N, N) and C.dtype == np.int32
        assert L.min() >= 1 and (L.max(axis=1) <= g["job_k"]).all()
        for i in range(len(KS)):
            want = sum((l[:, None] == l[None, :]).astype(np.int32) for l in L[i::len(KS)])
            assert np.array_equal(C[i], want), (key, KS[i])
            assert (np.diag(C[i]) == R).all()
