"""CPU side of the Brunet KL-divergence feature: the reference and the bound the GPU tests use (tests/kl_bound.py) are
coded correctly and are not vacuous, pinned against the fp64 oracle's own error.v figure, and the Python layer carries
the new fields."""
import numpy as np
import pytest

import kl_bound as kb

NOSTOP = 10 ** 6   # stopconv no restart reaches: the oracle runs to maxiter


def _ragged_A():
    A = np.asfortranarray(np.random.default_rng(603300).random((603, 300)) * 3.0)
    A[5, :] = 0.0
    A[:, 3] = 0.0
    return A


def _cases(golden):
    rng = np.random.default_rng(64005)
    yield "64x5 k=2", np.asfortranarray(rng.random((64, 5)) * 3.0), 2, 12, 7
    yield "gct k=2", golden["A_gct"], 2, 30, 11
    yield "gct k=5", golden["A_gct"], 5, 30, 12
    yield "ragged 603x300 k=7", _ragged_A(), 7, 12, 99
    sparse = np.asfortranarray(rng.random((333, 77)) * 3.0)
    sparse[rng.random(sparse.shape) < 0.3] = 0.0
    yield "333x77 k=7, 30 % zeros", sparse, 7, 12, 5


@pytest.fixture(scope="module")
def pinned(golden, oracle):
    """Per case: (what, A, W, H, error.v's last entry) with W, H the factors that entry is evaluated on.  NMF.div takes
    error.v[t] from the VP of iteration t's W update, i.e. from W of iteration t - 1 and H of iteration t."""
    out = []
    for what, A, k, T, seed in _cases(golden):
        m, n = A.shape
        W0, H0 = oracle.brunet_init(seed, m, n, k)
        Wp, _, tp = oracle.brunet(A, W0, H0, T - 1, NOSTOP)
        _, H, t, err = oracle.brunet(A, W0, H0, T, NOSTOP, want_error=True)
        assert tp == T - 1 and t == T and err.shape == (T,)
        out.append((what, A, Wp, H, float(err[-1])))
    return out


def test_bound_admits_the_oracle_and_rejects_1e9(pinned):
    for what, A, W, H, ev in pinned:
        d_s, bound = kb.div_and_bound(A, W, H)
        assert d_s > 0 and bound > 0, what
        assert float(kb.ref_kl_div(A, W, H)) == float(d_s)
        kb.check(ev, A, W, H, what + " oracle error.v", ref=(d_s, bound))
        # a plain fp64 evaluation of the same expression
        p = W @ H
        t = A * np.log((A + kb.EPS) / (p + kb.EPS)) - A + p
        kb.check(t.sum() / (float(A.shape[0]) * A.shape[1]), A, W, H, what + " numpy", ref=(d_s, bound))
        # not vacuous: a relative 1e-9 is outside, and so is anything not finite
        for off in (1e-9, -1e-9):
            assert not kb.within(float(d_s) * (1.0 + off), d_s, bound), (what, off, float(bound / d_s))
        assert not kb.within(float("nan"), d_s, bound) and not kb.within(float("inf"), d_s, bound)


def test_zero_entries_contribute_p(pinned):
    """Where a = 0 the term is exactly p: the reference over the zero row of the ragged case is sum(p) of that row."""
    what, A, W, H, _ = pinned[3]
    t, a, p, _ = kb.terms(A, W, H)
    assert np.all(a[5, :] == 0) and np.array_equal(t[5, :], p[5, :]) and np.array_equal(t[:, 3], p[:, 3])
    assert np.all(np.isfinite(t.astype(np.float64)))


def test_bound_formula_on_a_hand_case():
    """1 x 2, k = 1: a = (0, 2), p = (0.5, 1).  t = (0.5, 2 log(r) - 1) with r = (2 + eps) / (1 + eps)."""
    A = np.array([[0.0, 2.0]])
    W = np.array([[0.5]])
    H = np.array([[1.0, 2.0]])
    LD, u, eps = kb.LD, kb.LD(kb.U), kb.LD(kb.EPS)
    lg = np.log((LD(2) + eps) / (LD(1) + eps))
    t1 = LD(2) * lg - LD(1)
    d_s, bound = kb.div_and_bound(A, W, H)
    assert abs(d_s - (LD(0.5) + t1) / 2) < LD(1e-18)
    # E = u [(k + 6) a + (k + 3) p + (L + 3) a |log r|], k = 1, L = 2
    E = u * (7 * LD(0) + 4 * LD(0.5)) + u * (7 * LD(2) + 4 * LD(1) + 5 * LD(2) * lg)
    want = (E + 4 * u * (LD(0.5) + abs(t1))) / 2
    assert abs(bound - want) < LD(1e-30)


def test_log_ulp_measure():
    """The ulp measure the GPU test prints: numpy's own fp64 log is within one ulp; a value two ulps off reads as two."""
    x = np.random.default_rng(1).uniform(1e-3, 50.0, 20000)
    y = np.log(x)
    assert kb.log_ulp_error(x, y) <= 1.0
    y2 = y.copy()
    y2[7] = np.nextafter(np.nextafter(y2[7], np.inf), np.inf)
    assert 1.0 < kb.log_ulp_error(x, y2) <= 3.0


def test_python_layer_carries_the_new_fields():
    import dataclasses
    import inspect
    from nmfconsensus_amd import _lib
    from nmfconsensus_amd.brunet import BrunetEngine, NMF_div, nmfconsensus
    from nmfconsensus_amd.nmf import SweepResult
    names = {f.name for f in dataclasses.fields(SweepResult)}
    assert {"divergence", "best_restart", "best_divergence", "best_W", "best_H"} <= names
    for fn in (BrunetEngine.run, NMF_div, nmfconsensus):
        par = inspect.signature(fn).parameters
        assert par["want_divergence"].default is False and par["want_best"].default is False, fn
    assert {"nmfc_brunet_set_divergence", "nmfc_brunet_divergence", "nmfc_brunet_best"} <= set(_lib.EXPORTED)
    assert _lib.BK_DIV == 3
