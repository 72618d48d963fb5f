"""The numpy restatement of nmf_neals (tests/neals_ref.py) against the reference's own results
(tests/golden/golden_neals.npz, written by tests/golden/make_golden_neals.py), on the CPU.

Iteration counts must be equal, job for job.  For the jobs whose count is even (the only ones the reference can return
factors for) the reference's distance from the long-double restatement is printed per job ("NEALS|ref_dist|..."): it
is the yardstick tests/test_gpu_neals.py scales, and it must equal the figure the generator stored.
"""
import numpy as np
import pytest

import neals_ref as nr
from conftest import relfro


def jobs_of(mat, tolx):
    return [job for job in nr.golden_jobs()[2] if job["mat"] == mat and job["tolx"] == tolx]


def check(job):
    r = nr.neals(job["A"], job["W0"], job["cap"], TolX=job["TolX"], TolFun=job["TolX"], fixed=not job["tolx"])
    assert r["status"] == 0 and r["iters"] == job["iters"], (job["j"], r["iters"], job["iters"])
    if "H" in job:
        d = relfro(job["H"], r["H"])
        if "W" in job:
            d = max(d, relfro(job["W"], r["W"]))
        print(f"NEALS|ref_dist|job {job['j']}|mat={job['mat']} k={job['k']} seed={job['seed']} "
              f"{'tolx' if job['tolx'] else 'fixed'} iters={job['iters']}|{d:.3e}|stored {job['ref_dist']:.3e}")
        assert d <= 1e-9                       # the project's parity tolerance; measured 1e-14 .. 2e-10
        assert job["ref_dist"] >= d > 0        # the stored figure covers W too, whether the file holds that W or not
        assert np.array_equal(nr.labels(job["H"]), nr.labels(r["H"]))
        if "W" in job:
            # the W step alone, in long double, from the reference's H against the reference's W: the construction
            # test_gpu_neals.py uses for the reference's W where the file does not hold it.  It differs from the
            # reference's W by one double-precision W step's error, the kind of error ref_dist measures: 16 x that
            dc = relfro(nr.w_from_h(job["A"], job["H"]), job["W"])
            print(f"NEALS|w_from_h|job {job['j']}|{dc:.3e} of {max(16 * job['ref_dist'], 1e-13):.3e}")
            assert dc <= max(16 * job["ref_dist"], 1e-13)
        if "Hld" in job:
            assert np.array_equal(job["Hld"], r["H"])
    else:
        assert job["iters"] % 2 == 1 and job["ref_dist"] == -1.0


def test_golden_holds_the_issue_jobs():
    _, _, jobs = nr.golden_jobs()
    assert len(jobs) >= 47   # 56 asked for, at most one in six dropped by the generator
    assert {(j["mat"], j["k"]) for j in jobs} == {(0, k) for k in (2, 3, 4, 5)} | {(1, k) for k in (2, 3, 4, 5, 6)}
    assert any(j["tolx"] and j["iters"] < j["cap"] for j in jobs) and any(j["iters"] % 2 for j in jobs)


@pytest.mark.parametrize("mat", [0, 1])
def test_fixed_jobs(mat):
    for job in jobs_of(mat, 0):
        check(job)


@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_tolx_jobs(k):
    for job in jobs_of(0, 1):
        if job["k"] == k:
            check(job)


def test_double_and_long_double_forms_agree():
    """The plain-double run of the same code (the stand-in for the reference at odd counts in the GPU tests) against the
    long-double one: the size of a double-precision implementation's own error, printed."""
    _, A_pl, _ = nr.golden_jobs()
    rng = np.random.default_rng(3)
    for k in (2, 6):
        W0 = rng.random((300, k))
        a = nr.neals(A_pl, W0, 3, fixed=True)
        b = nr.neals(A_pl, W0, 3, fixed=True, dtype=np.float64)
        d = max(relfro(b["W"], a["W"]), relfro(b["H"], a["H"]))
        print(f"NEALS|double vs long double|k={k}|{d:.3e}")
        assert 0 < d <= 1e-11


def test_zero_pivot_status():
    _, A_pl, _ = nr.golden_jobs()
    W0 = np.random.default_rng(4).random((300, 3))
    W0[:, 1] = 0.0
    r = nr.neals(A_pl, W0, 5, fixed=True)
    assert (r["status"], r["iters"]) == (1, 1) and np.array_equal(r["W"], W0)
