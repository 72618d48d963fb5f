"""CPU side of the residual-norm feature: the bound the GPU tests use is coded correctly and is not vacuous, and the
Python result types carry and merge the new fields (tests/residual_bound.py, nmf.SweepResult,
distributed.merge_results)."""
import numpy as np

import residual_bound as rb
import widerange as wr


def _cases(golden):
    A, W0, H0 = wr.wide_case(1100, 72, 7, wr.SEED)
    W, H = wr.ref_mu(A, W0, H0, 2)
    yield "wide 1100x72 k=7 T=2", A, np.asfortranarray(W.astype(np.float64)), np.asfortranarray(H.astype(np.float64))
    for k in (2, 5):
        yield f"gct k={k} T=10", golden["A_gct"], golden[f"fixed_k{k}_T10_W"], golden[f"fixed_k{k}_T10_H"]
    yield "gct k=3 REF_COMPAT", golden["A_gct"], golden["refc_k3_W"], golden["refc_k3_H"]


def test_bound_admits_fp64_and_rejects_1e9(golden, oracle):
    for what, A, W, H in _cases(golden):
        m, n = A.shape
        norm_s, bound = rb.norm_and_bound(A, W, H)
        assert norm_s > 0 and bound > 0
        d = A - W @ H
        plain = np.sqrt((d * d).sum()) / np.sqrt(float(m) * n)
        rb.check(plain, A, W, H, what + " numpy")
        v, _ = oracle.calculate_norm(A, W, H)
        rb.check(v, A, W, H, what + " oracle calculateNorm")
        # not vacuous: a relative 1e-9 is far outside
        for off in (1e-9, -1e-9):
            assert not rb.within(float(norm_s) * (1.0 + off), norm_s, bound), (what, off)
        assert not rb.within(float("nan"), norm_s, bound)
        assert bound < 1e-11 * norm_s, (what, float(bound / norm_s))


def test_bound_formula_on_a_hand_case():
    """2 x 2, k = 1, exact in binary: A - W H = [[1, 0], [2, -2]], norm* = sqrt(9 / 4); E = 3 u (|A| + |W||H|)."""
    A = np.array([[2.0, 2.0], [4.0, 2.0]])
    W = np.array([[1.0], [2.0]])
    H = np.array([[1.0, 2.0]])
    norm_s, bound = rb.norm_and_bound(A, W, H)
    assert float(norm_s) == 1.5
    E = 3 * wr.U * np.array([[3.0, 4.0], [6.0, 6.0]])
    want = np.sqrt((E * E).sum() / 4) + 6 * wr.U * 1.5
    assert abs(float(bound) - want) < 1e-30


def _part(ks, R, jb, je, dnorm, best):
    from nmfconsensus_amd.nmf import SweepResult
    nj = je - jb
    return SweepResult(ks=ks, R=R, n=3, counts=None, consensus=None, labels=np.zeros((nj, 3), np.int32),
                       iters=np.arange(jb, je, dtype=np.int32), stopped_early=np.zeros(nj, np.int32), job_begin=jb,
                       job_end=je, dnorm=None if dnorm is None else np.array(dnorm, dtype=np.float64), best=best)


def test_sweepresult_has_dnorm_and_best():
    from nmfconsensus_amd.nmf import SweepResult
    import dataclasses
    names = {f.name for f in dataclasses.fields(SweepResult)}
    assert {"dnorm", "best"} <= names
    r = _part([2, 3], 1, 0, 2, None, None)
    assert r.dnorm is None and r.best is None


def test_merge_results_dnorm_and_best():
    from nmfconsensus_amd.distributed import merge_results
    b = lambda job, dn: dict(job=job, dnorm=dn, W=np.full((1, 1), float(job)), H=np.full((1, 1), float(job)))  # noqa: E731
    ks = [2, 3]
    # jobs 0..5: k = 2 at 0, 2, 4 and k = 3 at 1, 3, 5.  k = 2: 0.5 at job 0 and again at job 4 (a tie across parts: the
    # lower id wins); k = 3: the minimum sits in the last part
    p0 = _part(ks, 3, 0, 1, [0.5], {2: b(0, 0.5)})
    p1 = _part(ks, 3, 1, 4, [0.9, 0.7, 0.8], {3: b(3, 0.8), 2: b(2, 0.7)})
    p2 = _part(ks, 3, 4, 6, [0.5, 0.25], {2: b(4, 0.5), 3: b(5, 0.25)})
    for parts in ([p0, p1, p2], ):
        r = merge_results(parts)
        assert r.dnorm.dtype == np.float64 and np.array_equal(r.dnorm, [0.5, 0.9, 0.7, 0.8, 0.5, 0.25])
        assert (r.job_begin, r.job_end) == (0, 6)
        assert sorted(r.best) == [2, 3]
        assert r.best[2]["job"] == 0 and r.best[2]["dnorm"] == 0.5 and r.best[2]["W"][0, 0] == 0.0
        assert r.best[3]["job"] == 5 and r.best[3]["dnorm"] == 0.25 and r.best[3]["H"][0, 0] == 5.0
    # the order of the parts does not decide a tie
    from nmfconsensus_amd.distributed import merge_best
    assert merge_best([p2, p1, p0])[2]["job"] == 0
    # a part without residuals: no merged dnorm; parts without best: none
    q = _part(ks, 3, 4, 6, None, None)
    r = merge_results([p0, p1, q])
    assert r.dnorm is None and r.best[3]["job"] == 3
    assert merge_results([_part(ks, 3, 0, 1, [1.0], None), _part(ks, 3, 1, 6, [1.0] * 5, None)]).best is None
    # one part is returned as it is
    assert merge_results([p1]) is p1
