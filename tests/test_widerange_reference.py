"""The inputs and the long-double references of tests/test_gpu_widerange.py, pinned before any GPU sees them.  No GPU.

For every (shape, k) the GPU tests run (widerange.mu_shapes / kl_shapes): the fp64 oracle passes the componentwise check
against the long-double reference at T = 1 and T = 2 (4..116 u against bounds of 34..690 960 u), and the data meets the conditions that
make the check worth running: a fifth of the rows of W and of the columns of H below what the relative Frobenius bar of
1e-9 can see, MU denominators on both sides of 1e-9 on the H side and on the W side, no value near the underflow or
overflow limits (so every zero is structural), and for KL brunet.hip's admitted domain.  A numpy restatement of the MU
update without DIV_BY_ZERO_AVOIDANCE, and one with the constant doubled, fail the check by many orders.
The Euclidean NMF() cases (widerange.EUCLID_BATCHES): positive denominators and normal intermediates, the rule's products
on both sides of 2^-52, the elements that are exactly 2^-52, and the fp64 Gram form of tests/euclid_ref.py inside the
bound (4..45 u against bounds of 207..256 980 u); eps added twice or before the divide, or the MU rule's 1e-9 in the
denominator, miss it by 1e15 u and more."""
import numpy as np
import pytest

import widerange as wr
from conftest import relfro

MU = wr.mu_shapes()
KL = wr.kl_shapes()
# one case per MU path runs T = 40 against the oracle on the GPU (zero pattern, relfro < 1e-9)
T40 = wr.T40_CASES


def ids(shapes):
    return ["x".join(str(v) for v in s) for s in shapes]


def test_bound_recursion_values():
    assert wr.bound_u(1000, 40, 5, 1) == (2013, 6132)
    bh, bw = wr.bound_u(1000, 40, 5, 2)
    assert (bh, bw) == (3 * 6132 + 2 * 2013 + 2013, 3 * (3 * 6132 + 2 * 2013 + 2013) + 2 * 6132 + 93)
    assert 80000 < bw < 90000
    # the largest bound any test uses still sits far below the 1e-9 of the norm-wise bar
    assert max(max(wr.bound_u(m, n, k, 2)) for m, n, k in MU + KL + wr.euclid_shapes()) * wr.U < 1e-10


def test_cw_check_rejects():
    ref = np.array([1.0, 0.0, 1e-30, 3.0], dtype=wr.LD)
    assert wr.cw_check(np.array([1.0, 0.0, 1e-30, 3.0]), ref, 1) <= 1
    with pytest.raises(AssertionError):
        wr.cw_check(np.array([1.0, 1e-300, 1e-30, 3.0]), ref, 10)    # a value where the reference has a zero
    with pytest.raises(AssertionError):
        wr.cw_check(np.array([1.0, 0.0, 0.0, 3.0]), ref, 10)         # a zero where the reference has a value
    with pytest.raises(AssertionError):
        wr.cw_check(np.array([1.0, 0.0, 1.0000001e-30, 3.0]), ref, 10)   # a small entry off by 1e-7: invisible to a norm
    with pytest.raises(AssertionError):
        wr.cw_check(np.array([1.0, 0.0, np.nan, 3.0]), ref, 10)


def test_recipe():
    m, n, k = 1100, 72, 7
    A, W0, H0 = wr.case("mu", m, n, k)
    assert A.flags["F_CONTIGUOUS"] and A.shape == (m, n) and W0.shape == (m, k) and H0.shape == (k, n)
    assert np.all(A[5 % m, :] == 0) and np.all(A[:, 3 % n] == 0) and np.all(H0[1, :] == 0)
    assert 0.25 < np.mean(A == 0) < 0.40 and 0.05 < np.mean(W0 == 0) < 0.15
    rows = np.array([np.max(A[i, :]) for i in range(m)])
    edge = wr.edge_rows(m)
    assert m - 1 in edge and set(range(1088, 1100)) <= set(edge)   # the last partial 16-row block of m = 1100
    rest = np.setdiff1d(np.arange(m), edge + [5])
    assert rows[edge].max() < np.median(rows[rest])
    # the jobs of a batch share A, have their own streams, and W0 scaled by 2^(-8 (job % 5))
    assert wr.case("mu", m, n, k, 3)[0] is A
    W3 = wr.case("mu", m, n, k, 3)[1]
    assert not np.array_equal(W3 * 2.0 ** 24, W0) and np.median(W3[W3 > 0]) < np.median(W0[W0 > 0]) * 2.0 ** -16
    for a, b in zip(wr.wide_case(m, n, k, wr.SEED), (A, W0, H0)):
        assert np.array_equal(a, b)
    _, Wk, Hk = wr.case("kl", 603, 300, 5)
    assert np.all(Wk > 0) and np.all(Hk > 0)


@pytest.mark.parametrize("m,n,k", MU, ids=ids(MU))
def test_mu_case(oracle, m, n, k):
    A, W0, H0 = wr.case("mu", m, n, k)
    c = wr.measure("mu", m, n, k)
    print(f"mu {m}x{n} k={k}: " + " ".join(f"{a}={b:.3g}" for a, b in c.items()))
    assert c["belowW"] >= 0.20 and c["belowH"] >= 0.20, c
    for side in ("H", "W"):
        assert c[f"{side}den_lo"] >= 0.10 and c[f"{side}den_hi"] >= 0.10, (side, c)
    assert 1e-250 < c["min"] and c["max"] < 1e250, c
    ref = wr.reference("mu", m, n, k)
    for T in (1, 2):
        Wo, Ho, it = oracle.nmf_mu(A, W0, H0, T, 0)
        bh, bw = wr.bound_u(m, n, k, T)
        eh = wr.cw_check(Ho, ref[T][1], bh, f"oracle H {m}x{n} k={k} T={T}")
        ew = wr.cw_check(Wo, ref[T][0], bw, f"oracle W {m}x{n} k={k} T={T}")
        print(f"  oracle T={T}: H {eh:.0f} u of {bh}, W {ew:.0f} u of {bw}")
        assert it == T


@pytest.mark.parametrize("m,n,k", KL, ids=ids(KL))
def test_kl_case(oracle, m, n, k):
    A, W0, H0 = wr.case("kl", m, n, k)
    assert A.max() <= 2.0 ** 64 and A.sum() <= 2.0 ** 100
    for job in range(64):   # more than any batch the GPU tests run
        _, W, H = wr.case("kl", m, n, k, job)
        assert 2.0 ** -60 <= min(W.min(), H.min()) and max(W.max(), H.max()) <= 2.0 ** 60, job
    c = wr.measure("kl", m, n, k)
    print(f"kl {m}x{n} k={k}: " + " ".join(f"{a}={b:.3g}" for a, b in c.items()))
    assert c["belowW"] >= 0.20 and c["belowH"] >= 0.20, c
    assert 1e-250 < c["min"] and c["max"] < 1e250, c
    ref = wr.reference("kl", m, n, k)
    for T in (1, 2):
        Wo, Ho, it = oracle.brunet(A, W0, H0, T, 10 ** 6)
        bh, bw = wr.bound_u(m, n, k, T)
        eh = wr.cw_check(Ho, ref[T][1], bh, f"oracle H {m}x{n} k={k} T={T}")
        ew = wr.cw_check(Wo, ref[T][0], bw, f"oracle W {m}x{n} k={k} T={T}")
        print(f"  oracle T={T}: H {eh:.0f} u of {bh}, W {ew:.0f} u of {bw}")
        assert it == T


@pytest.mark.parametrize("kind,m,n,k", [("mu", 1100, 72, 16), ("mu", 1000, 40, 9), ("kl", 603, 300, 10)])
def test_scaled_jobs_of_a_batch(oracle, kind, m, n, k):
    """Jobs 1..4 of a batch (W0 times 2^-8 .. 2^-32, their own streams): the oracle within the bound, no underflow."""
    wr.prefetch(kind, m, n, k, range(1, 5))
    for job in range(1, 5):
        A, W0, H0 = wr.case(kind, m, n, k, job)
        ref = wr.reference(kind, m, n, k, job)
        for T in (1, 2):
            Wo, Ho, _ = oracle.nmf_mu(A, W0, H0, T, 0) if kind == "mu" else oracle.brunet(A, W0, H0, T, 10 ** 6)
            bh, bw = wr.bound_u(m, n, k, T)
            eh = wr.cw_check(Ho, ref[T][1], bh, f"job {job} H T={T}")
            ew = wr.cw_check(Wo, ref[T][0], bw, f"job {job} W T={T}")
            pos = np.concatenate([x[x > 0].ravel() for x in ref[T]])
            assert 1e-250 < pos.min() and pos.max() < 1e250
            print(f"{kind} {m}x{n} k={k} job {job} T={T}: H {eh:.0f} u of {bh}, W {ew:.0f} u of {bw}")


@pytest.mark.parametrize("m,n,k", T40, ids=ids(T40))
def test_forty_iterations_do_not_underflow(oracle, m, n, k):
    """The T = 40 run the GPU test compares zero patterns on: every positive value of the oracle stays far from the
    underflow limit, so a zero after 40 iterations is structural (old == 0 || num == 0), never a flushed value."""
    A, W0, H0 = wr.case("mu", m, n, k)
    W, H, _ = oracle.nmf_mu(A, W0, H0, 40, 0)
    pos = np.concatenate([W[W > 0], H[H > 0]])
    print(f"T=40 {m}x{n} k={k}: positive values in [{pos.min():.2e}, {pos.max():.2e}]")
    assert np.isfinite(W).all() and np.isfinite(H).all()
    assert 1e-250 < pos.min() and pos.max() < 1e250
    # the zero pattern is that of the first update: nothing joins it later
    ref = wr.reference("mu", m, n, k)
    assert np.array_equal(W == 0, ref[1][0] == 0) and np.array_equal(H == 0, ref[1][1] == 0)


def mu_fp64(A, W, H, T, eps):
    """The MU update restated in numpy fp64 with the constant `eps` in place of DIV_BY_ZERO_AVOIDANCE."""
    W, H = W.copy(), H.copy()
    for _ in range(T):
        num, den = W.T @ A, (W.T @ W) @ H
        H = np.where((H == 0) | (num == 0), 0.0, H * (num / np.where(den + eps > 0, den + eps, 1.0)))
        num, den = A @ H.T, W @ (H @ H.T)
        W = np.where((W == 0) | (num == 0), 0.0, W * (num / np.where(den + eps > 0, den + eps, 1.0)))
    return W, H


@pytest.mark.parametrize("m,n,k", [(1000, 40, 5), (1100, 72, 7), (130, 17, 3)])
def test_constant_sensitivity(m, n, k):
    """Dropping or doubling DIV_BY_ZERO_AVOIDANCE fails the componentwise check at T = 1 on the wide case by many
    orders; on the suite's uniform data it moves W and H by a few 1e-9 relative Frobenius after 24 iterations, the
    thin margin of the norm-wise bar (printed, not asserted)."""
    A, W0, H0 = wr.case("mu", m, n, k)
    ref = wr.reference("mu", m, n, k)[1]
    bh, bw = wr.bound_u(m, n, k, 1)
    W, H = mu_fp64(A, W0, H0, 1, 1e-9)
    wr.cw_check(H, ref[1], bh, "restatement H"), wr.cw_check(W, ref[0], bw, "restatement W")
    for name, eps in (("dropped", 0.0), ("doubled", 2e-9)):
        W, H = mu_fp64(A, W0, H0, 1, eps)
        (zh, eh), (zw, ew) = wr.cw_error(H, ref[1]), wr.cw_error(W, ref[0])
        print(f"constant {name} on wide {m}x{n} k={k}: H off by {eh:.3g} u (bound {bh}), W by {ew:.3g} u (bound {bw})")
        assert zh == 0 and zw == 0            # the zero rule is untouched: only the values move
        assert eh > 1e6 * bh and ew > 1e6 * bw
    rng = np.random.default_rng(31 * m + n)
    Au = np.asfortranarray(rng.random((m, n)) * 2.0 + 0.05)
    Wu, Hu = rng.random((m, k)) + 0.01, rng.random((k, n)) + 0.01
    Wt, Ht = mu_fp64(Au, Wu, Hu, 24, 1e-9)
    for name, eps in (("dropped", 0.0), ("doubled", 2e-9)):
        W, H = mu_fp64(Au, Wu, Hu, 24, eps)
        print(f"constant {name} on uniform {m}x{n} k={k}, T=24: relfro W {relfro(W, Wt):.2e} H {relfro(H, Ht):.2e} "
              f"(the bar is 1e-9)")


# ---- the Euclidean NMF() rule (widerange.EUCLID_BATCHES) ----------------------------------------------------------------

EUC = wr.euclid_shapes()
EUC_R = {(m, n, k): max(R for mm, nn, ks, R, _ in wr.EUCLID_BATCHES if (mm, nn) == (m, n) and k in ks) for m, n, k in EUC}


def euclid_fp64(A, W0, H0, T):
    """T updates of the fp64 Gram form of tests/euclid_ref.py."""
    import euclid_ref as er
    W, H = np.array(W0), np.array(H0)
    for _ in range(T):
        W, H = er._update(np.asarray(A), W, H, np.float64(er.EPS), "gram")
    return W, H


def euclid_exact_eps(m, n, W0, H0, T):
    """(mask of W, mask of H) of the elements the rule leaves at exactly eps after T updates: the all-zero row 5 % m of
    A (a row of W), its all-zero column 3 % n (a column of H) and, after the first update, every zero of W0 and H0."""
    zw, zh = (W0 == 0) & (T == 1), (H0 == 0) & (T == 1)
    zw[5 % m, :] = True
    zh[:, 3 % n] = True
    return zw, zh


def test_euclid_recipe():
    m, n, k = 1100, 72, 7
    A, W0, H0 = wr.case("euclid", m, n, k)
    assert A.flags["F_CONTIGUOUS"] and A.shape == (m, n) and W0.shape == (m, k) and H0.shape == (k, n)
    assert np.all(A[5 % m, :] == 0) and np.all(A[:, 3 % n] == 0) and 0.25 < np.mean(A == 0) < 0.40
    # the same draws as the MU matrix at another scale
    assert np.allclose(A, wr.case("mu", m, n, k)[0] * (wr.ALPHA["euclid"] / wr.ALPHA["mu"]), rtol=1e-14, atol=0)
    W3 = wr.case("euclid", m, n, k, 3)[1]
    assert wr.case("euclid", m, n, k, 3)[0] is A
    assert np.median(W3[W3 > 0]) < np.median(W0[W0 > 0]) * 2.0 ** -16
    assert wr.EUCLID_EPS == 2.0 ** -52 and wr.EUCLID_EPS == np.finfo(np.float64).eps
    # every RULE_EUCLID form of the A h^T kernel has a batch that is there for it
    assert set(wr.EUCLID_FORMS) == wr.EUCLID_ALL_FORMS
    for a, b in wr.EUCLID_SAME_BITS:
        assert wr.EUCLID_BATCHES[a][:4] == wr.EUCLID_BATCHES[b][:4] and wr.EUCLID_BATCHES[a][4] != wr.EUCLID_BATCHES[b][4]


@pytest.mark.parametrize("m,n,k", EUC, ids=ids(EUC))
def test_euclid_case(m, n, k):
    """(a) denominators positive, intermediates zero or normal; (b) eps decides on both sides; (c) the exact-eps sets;
    (d) the fp64 Gram form inside the bound.  Job 0 for all four; the scaled jobs of the batch for (a), (c) and (d)."""
    tiny, huge = np.finfo(np.float64).tiny, np.finfo(np.float64).max
    wr.prefetch("euclid", m, n, k, range(EUC_R[(m, n, k)]))
    for job in range(EUC_R[(m, n, k)]):
        A, W0, H0 = wr.case("euclid", m, n, k, job)
        for X in (W0, H0):
            assert 0.03 < np.mean(X == 0) < 0.18   # about 10 %
            assert not (X == 0).all(axis=0).any() and not (X == 0).all(axis=1).any()
        # (a)
        c = wr.measure_euclid(A, W0, H0)
        print(f"euclid {m}x{n} k={k} job {job}: " + " ".join(f"{a}={b:.3g}" for a, b in c.items()))
        assert c["Hden_min"] > 0 and c["Wden_min"] > 0, c
        assert tiny <= c["min"] and c["max"] <= huge, c
        # (b)
        if job == 0:
            for side in "HW":
                assert c[f"{side}lo"] >= 0.05 and c[f"{side}hi"] >= 0.25, (side, c)
        # (c)
        assert (W0 == 0).any() and (H0 == 0).any()
        ref = wr.reference("euclid", m, n, k, job)
        for T in (1, 2):
            Wr, Hr = ref[T]
            zw, zh = euclid_exact_eps(m, n, W0, H0, T)
            assert zw[5 % m, :].all() and zh[:, 3 % n].all()
            assert np.all(Wr[zw] == wr.LD(wr.EUCLID_EPS)) and np.all(Hr[zh] == wr.LD(wr.EUCLID_EPS))
            assert np.all(Wr >= wr.LD(wr.EUCLID_EPS)) and np.all(Hr >= wr.LD(wr.EUCLID_EPS))
            # (d)
            W, H = euclid_fp64(A, W0, H0, T)
            bh, bw = wr.bound_u(m, n, k, T)
            eh = wr.cw_check(H, Hr, bh, f"fp64 Gram form H {m}x{n} k={k} job {job} T={T}")
            ew = wr.cw_check(W, Wr, bw, f"fp64 Gram form W {m}x{n} k={k} job {job} T={T}")
            print(f"  fp64 Gram form job {job} T={T}: H {eh:.0f} u of {bh}, W {ew:.0f} u of {bw}")
            assert np.all(W[zw] == wr.EUCLID_EPS) and np.all(H[zh] == wr.EUCLID_EPS)


def euclid_mutant(A, W0, H0, which):
    """One fp64 update with the rule got wrong in the ways a kernel could get it wrong."""
    eps = wr.EUCLID_EPS
    num, den = W0.T @ A, (W0.T @ W0) @ H0
    H = H0 * (num / (den + 1e-9)) + eps if which == "mu-constant" else H0 * (num / den) + eps
    num, den = A @ H.T, W0 @ (H @ H.T)
    if which == "eps-twice":
        W = (W0 * num) / den + eps + eps
    elif which == "eps-before-divide":
        W = (W0 * num + eps) / den
    else:
        W = (W0 * num) / den + eps
    return W, H


@pytest.mark.parametrize("m,n,k", [(97, 33, 5), (200, 60, 4), (1100, 72, 7)])
def test_euclid_constant_sensitivity(m, n, k):
    """eps added twice or before the divide (W), or the MU rule's 1e-9 in the H denominator: each misses the bound at
    T = 1 on the wide case by orders; the restatement without a mutation passes."""
    A, W0, H0 = wr.case("euclid", m, n, k)
    Wr, Hr = wr.reference("euclid", m, n, k)[1]
    bh, bw = wr.bound_u(m, n, k, 1)
    W, H = euclid_mutant(A, W0, H0, None)
    wr.cw_check(H, Hr, bh, "restatement H"), wr.cw_check(W, Wr, bw, "restatement W")
    for which, side in (("eps-twice", "W"), ("eps-before-divide", "W"), ("mu-constant", "H")):
        W, H = euclid_mutant(A, W0, H0, which)
        _, err = wr.cw_error(H, Hr) if side == "H" else wr.cw_error(W, Wr)
        bound = bh if side == "H" else bw
        print(f"euclid {which} on wide {m}x{n} k={k}: {side} off by {err:.3g} u (bound {bound})")
        assert err > 1e6 * bound


# ---- the KL kernels at the corners of their domain (widerange.CORNER_*) ------------------------------------------------

CORNER = [(kind, m, n, k) for kind, m, n, ks in wr.CORNER_CASES for k in ks]


@pytest.mark.parametrize("kind,m,n,k", CORNER, ids=[f"{c[0]}-{c[1]}x{c[2]}-k{c[3]}" for c in CORNER])
def test_kl_corner_oracle_in_bound(oracle, kind, m, n, k):
    """The fp64 oracle passes the componentwise bound at T = 1 and 2 on the four factor-scale combinations, and the
    inputs sit where nmfc_brunet_create / nmfc_brunet_run admit them."""
    A = wr.case(kind, m, n, k)[0]
    assert A.min() >= 0 and A.max() <= 2.0 ** 64 and A.sum() <= 2.0 ** 100
    if kind == "kl-top":
        assert A.max() == 2.0 ** 64 and 0.2 < np.mean(A == 0) < 0.4
    elif kind == "kl-tiny":
        assert 2.0 ** -201 <= A.min() and A.max() < 2.0 ** -200
    else:
        e = np.frexp(A)[1]
        assert e.min() <= -50 and e.max() >= 55 and A.min() >= 2.0 ** -60
    wr.prefetch(kind, m, n, k, range(4))
    for job in range(4):
        _, W0, H0 = wr.case(kind, m, n, k, job)
        ew, eh = wr.CORNER_SIGNS[job]
        for X, ex in ((W0, ew), (H0, eh)):
            assert 2.0 ** (ex - 1) <= X.min() and X.max() < 2.0 ** ex and 2.0 ** -60 <= X.min() and X.max() <= 2.0 ** 60
        ref = wr.reference(kind, m, n, k, job)
        for T in (1, 2):
            Wo, Ho, it = oracle.brunet(A, W0, H0, T, 10 ** 6)
            bh, bw = wr.bound_u(m, n, k, T)
            eh_ = wr.cw_check(Ho, ref[T][1], bh, f"oracle H {kind} {m}x{n} k={k} job {job} T={T}")
            ew_ = wr.cw_check(Wo, ref[T][0], bw, f"oracle W {kind} {m}x{n} k={k} job {job} T={T}")
            print(f"{kind} {m}x{n} k={k} job {job} T={T}: H {eh_:.0f} u of {bh}, W {ew_:.0f} u of {bw}")
            assert it == T


CORNER_RANGE = [(kind, m, n, k) for kind, m, n, ks in wr.CORNER_CASES for k in ks if k in (2, 5, 16)]


@pytest.mark.parametrize("kind,m,n,k", CORNER_RANGE, ids=[f"{c[0]}-{c[1]}x{c[2]}-k{c[3]}" for c in CORNER_RANGE])
def test_kl_corner_reference_stays_in_range(kind, m, n, k):
    """Over the T = 40 the GPU test runs: every VP, W and H of the long-double reference is finite and normal, and any
    five VP values of the four factor-scale combinations (one batched reciprocal can hold restarts of all four) have a
    product inside [2^-1021, 2^1021], the contract of brunet.hip's recip_batch."""
    from concurrent.futures import ThreadPoolExecutor
    A = wr.case(kind, m, n, k)[0]
    with ThreadPoolExecutor(4) as ex:
        runs = list(ex.map(lambda job: wr.ref_kl_range(A, *wr.case(kind, m, n, k, job)[1:], wr.CORNER_T), range(4)))
    tiny, huge = np.finfo(np.float64).tiny, np.finfo(np.float64).max
    vlo, vhi = min(r[2][0] for r in runs), max(r[2][1] for r in runs)
    xlo, xhi = min(r[3][0] for r in runs), max(r[3][1] for r in runs)
    print(f"{kind} {m}x{n} k={k}, T={wr.CORNER_T}: VP in [2^{float(np.log2(vlo)):.1f}, 2^{float(np.log2(vhi)):.1f}], "
          f"W and H in [2^{float(np.log2(xlo)):.1f}, 2^{float(np.log2(xhi)):.1f}]")
    for W, H, _, _ in runs:
        assert np.isfinite(W).all() and np.isfinite(H).all()
    assert tiny <= vlo and vhi <= huge and tiny <= xlo and xhi <= huge
    assert 5 * float(np.log2(vlo)) >= -1021 and 5 * float(np.log2(vhi)) <= 1021
    # the first update's VP values of the four combinations lie some 2^236 apart
    first = [wr.case(kind, m, n, k, job)[1] @ wr.case(kind, m, n, k, job)[2] for job in (0, 3)]
    assert np.log2(first[0].min() / first[1].max()) > 232
