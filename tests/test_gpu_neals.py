"""libnmf's nmf_neals (normal-equation ALS) on the MFMA engine: Engine.run(neals=True), the nmf_neals drop-in, doNMF.

The kernels solve both k x k systems with the LU factors (partial pivoting, forward and back substitution per sample
and per gene row), never with an explicit inverse; test_badly_scaled_gram is the case where the two would differ.

Bounds.  Against the reference's own results (tests/golden/golden_neals.npz; the reference returns factors only after
even iteration counts): 1e-9 relative Frobenius, the project's parity tolerance.  Against the long-double restatement
(tests/neals_ref.py): 16 x the distance a double-precision CPU implementation has from that restatement on the same job,
floor 1e-13 -- the reference itself where the golden file has its factors (job["ref_dist"], printed by the generator and
by test_neals_reference.py), the plain-double numpy run of the restatement's code where it has none (odd counts, other
shapes).  Both sides put a backward-stable solve behind products that differ only in summation order, so their errors
share the factor cond(G) u and differ by a small constant; 16 covers split-K sums against a CPU BLAS's blocking.
Lines starting "NEALS|" print each figure beside its bound.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

import neals_ref as nr
import residual_bound as rb
from conftest import relfro

pytestmark = pytest.mark.gpu

FIXED, TOLX_RULE = 0, 3
TOL_REF = 1e-9
KNOBS = ("NMFC_AHTW_TILE", "NMFC_WTA_TILE", "NMFC_NARROW", "NMFC_NARROW_MAXB", "NMFC_REPACK_DIV")


@contextlib.contextmanager
def knobs(env):
    """The engine's knobs set to `env` (names without the NMFC_ prefix) and no other of KNOBS, restored after."""
    saved = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        for k, v in env.items():
            assert "NMFC_" + k in KNOBS, k
            os.environ["NMFC_" + k] = str(v)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def bound_of(dist):
    return max(16.0 * dist, 1e-13)


def dist_wh(r, ref):
    return max(relfro(r["W"], ref["W"]), relfro(r["H"], ref["H"]))


# ---- 1. golden parity ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fixed_restatement(j):
    job = nr.golden_jobs()[2][j]
    return nr.neals(job["A"], job["W0"], job["cap"], fixed=True)


@pytest.mark.parametrize("mat,tolx,cap", [(0, 0, 2), (0, 0, 10), (0, 1, 2000), (1, 0, 2), (1, 0, 4)])
def test_golden_parity(mat, tolx, cap):
    """Every golden job of one (matrix, stop rule, cap) in one batch from the reference's W0."""
    from nmfconsensus_amd.nmf import Engine
    jobs = [j for j in nr.golden_jobs()[2] if (j["mat"], j["tolx"], j["cap"]) == (mat, tolx, cap)]
    assert jobs
    A = jobs[0]["A"]
    ks = sorted({j["k"] for j in jobs})
    seeds = sorted({j["seed"] for j in jobs})
    grid = {(j["k"], j["seed"]): j for j in jobs}
    slots = [grid.get((ks[s % len(ks)], seeds[s // len(ks)])) for s in range(len(ks) * len(seeds))]
    rng = np.random.default_rng(1)   # a slot whose job the generator dropped runs from any W0 and is not compared
    W0 = [job["W0"] if job else rng.random((A.shape[0], ks[s % len(ks)])) for s, job in enumerate(slots)]
    with Engine(A) as eng:
        r = eng.run(ks, len(seeds), maxiter=cap, stop_rule=TOLX_RULE if tolx else FIXED, TolX=jobs[0]["TolX"],
                    TolFun=jobs[0]["TolX"], W_init=W0, want_factors=True, neals=True)
        assert eng.last_run_info()["small"] == 0
    assert r.neals_status is not None and not r.neals_status.any()
    compared = 0
    for s, job in enumerate(slots):
        if job is None:
            continue
        what = f"golden job {job['j']} mat={mat} k={job['k']} seed={job['seed']} {'tolx' if tolx else 'fixed'} cap={cap}"
        assert r.iters[s] == job["iters"], what
        assert r.stopped_early[s] == (1 if tolx and job["iters"] < cap else 0), what
        if "H" not in job:   # an odd count: the reference has no factors
            print(f"NEALS|golden|{what}|iters {r.iters[s]} (odd: count only)")
            continue
        compared += 1
        assert np.array_equal(r.labels[s], nr.labels(job["H"])), what
        # H against the reference's H; W against the reference's W: the stored one where the file holds it, and for
        # every even job the W one long-double W step away from the reference's H (neals_ref.w_from_h; the file holds W
        # for the FIXED jobs of one seed only, and test_neals_reference.py holds that construction to the stored ones)
        d_h = relfro(r.H[s], job["H"])
        d_w = relfro(r.W[s], nr.w_from_h(job["A"], job["H"]))
        if "W" in job:
            d_w = max(d_w, relfro(r.W[s], job["W"]))
        d_ref = max(d_h, d_w)
        if tolx:
            d_ld = relfro(r.H[s], job["Hld"])
        else:
            d_ld = dist_wh(dict(W=r.W[s], H=r.H[s]), fixed_restatement(job["j"]))
        print(f"NEALS|golden|{what}|iters {r.iters[s]}|vs reference H {d_h:.3e} W {d_w:.3e} of {TOL_REF:.0e}|"
              f"vs restatement {d_ld:.3e} of {bound_of(job['ref_dist']):.3e} (ref_dist {job['ref_dist']:.3e})")
        assert d_ref <= TOL_REF, what
        assert d_ld <= bound_of(job["ref_dist"]), what
    assert compared >= len(jobs) // 2


# ---- 2. one update, both sides, every form -------------------------------------------------------------------------

KS2, R2 = [2, 3, 4, 5, 6], 7
NARROW_BITS = {}   # (m, n, T) -> the "narrow" arm's result, for the "narrow_off" arm to compare with


@functools.lru_cache(maxsize=None)
def case2(m, n):
    """(A, job ranks, W0 per job, {T: [(long double run, its distance from the plain-double run)]}) for T = 1, 2."""
    from nmfconsensus_amd.synthetic import planted_matrix
    A = planted_matrix(m, n)
    jk = [KS2[j % len(KS2)] for j in range(len(KS2) * R2)]
    rng = np.random.default_rng(100 * m + n)
    W0 = [rng.random((m, k)) for k in jk]
    refs = {}
    for T in (1, 2):
        refs[T] = []
        for w0 in W0:
            ld = nr.neals(A, w0, T, fixed=True)
            db = nr.neals(A, w0, T, fixed=True, dtype=np.float64)
            refs[T].append((ld, dist_wh(db, ld)))
    return A, jk, W0, refs


@pytest.mark.parametrize("arm", ["default", "tile128", "tile64", "narrow", "narrow_off"])
@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("m,n", [(130, 41), (300, 70), (200, 61)])
def test_one_update_every_form(m, n, T, arm):
    """FIXED 1 and 2 iterations, k = 2..6 with R = 7 (16-column blocks hold restarts of different ranks, the last one is
    partly padding), on a padded gene tile with n no multiple of 8 or of the K stage (130 x 41), on 300 x 70 and on
    200 x 61.  By plan_chunk's host rule (the KHALF instantiations when n_pad - n >= 8, n_pad = n rounded up to 32) the
    first two shapes launch the KHALF forms (64 - 41 = 23, 96 - 70 = 26) and the third the full-stage ones (64 - 61 = 3);
    the run info has no counter for that, so it is the host rule restated, not observed.  Arms: the default tiles; NMFC_AHTW_TILE
    forcing the 128- and the 64-gene A h^T tile; "narrow": a shard of the first eight jobs, which fits three 16-column
    blocks, the condition under which the engine takes the narrow W^T A and A h^T forms (NMFC_NARROW left at its
    default, on); "narrow_off": the same shard with NMFC_NARROW=0, which must take no narrow form and give the narrow
    arm's bits.  The run info proves per arm which forms ran."""
    from nmfconsensus_amd.nmf import Engine
    A, jk, W0, refs = case2(m, n)
    env = {"tile128": {"AHTW_TILE": 128}, "tile64": {"AHTW_TILE": 64}, "narrow_off": {"NARROW": 0}}.get(arm, {})
    je = 8 if arm.startswith("narrow") else len(jk)
    with knobs(env), Engine(A) as eng:
        r = eng.run(KS2, R2, maxiter=T, stop_rule=FIXED, W_init=W0[:je], job_end=je, want_factors=True, neals=True,
                    want_counts=False)
        info = eng.last_run_info()
    assert info["small"] == 0
    if arm == "narrow":
        assert info["ahtw_narrow"] == T and info["wta_narrow"] == T, info
        NARROW_BITS[(m, n, T)] = r
    elif arm == "narrow_off":
        assert info["ahtw_narrow"] == 0 and info["wta_narrow"] == 0 and info["ahtw_128"] + info["ahtw_64"] == T, info
        nb = NARROW_BITS[(m, n, T)]   # the "narrow" arm of this case ran just before (parametrize order)
        assert all(np.array_equal(r.W[j], nb.W[j]) and np.array_equal(r.H[j], nb.H[j]) for j in range(je))
    elif arm == "default":
        assert info["ahtw_128"] + info["ahtw_64"] == T, info
    else:
        assert info["ahtw_128" if arm == "tile128" else "ahtw_64"] == T, info
    assert np.all(r.iters == T) and not r.neals_status.any() and not r.stopped_early.any()
    worst = 0.0
    for j in range(je):
        ld, yard = refs[T][j]
        d = dist_wh(dict(W=r.W[j], H=r.H[j]), ld)
        worst = max(worst, d / bound_of(yard))
        assert d <= bound_of(yard) and d <= TOL_REF, (j, jk[j], d, yard)
        assert np.all(r.H[j] >= 0) and not np.signbit(r.H[j]).any()   # the H clamp gives +0.0
    print(f"NEALS|one update|{m}x{n} T={T} {arm}|worst distance / bound {worst:.3f}|{info}")


# ---- 3. placement changes no bit ------------------------------------------------------------------------------------

def same(a, b, j, jb=0):
    return (np.array_equal(a.W[j], b.W[j - jb]) and np.array_equal(a.H[j], b.H[j - jb]) and
            a.iters[j] == b.iters[j - jb] and a.stopped_early[j] == b.stopped_early[j - jb] and
            a.neals_status[j] == b.neals_status[j - jb] and np.array_equal(a.labels[j], b.labels[j - jb]))


def test_placement_changes_no_bit(golden):
    """One gct sweep, k = 2..5, R = 6, under TolX (cap 400): whole, as two shards, every job alone, and with a repack at
    every stop."""
    from nmfconsensus_amd.nmf import Engine
    A, ks, R = golden["A_gct"], [2, 3, 4, 5], 6
    kw = dict(maxiter=400, seed=321, stop_rule=TOLX_RULE, TolX=1e-4, want_factors=True, neals=True, want_counts=False)
    with Engine(A) as eng:
        whole = eng.run(ks, R, **kw)
        shards = [eng.run(ks, R, job_begin=0, job_end=11, **kw), eng.run(ks, R, job_begin=11, **kw)]
        alone = [eng.run(ks, R, job_begin=j, job_end=j + 1, **kw) for j in range(len(ks) * R)]
    with knobs({"REPACK_DIV": 1000}), Engine(A) as eng:
        packed = eng.run(ks, R, check_every=1, **kw)
        info = eng.last_run_info()
    assert info["repacks"] >= 2, info
    stops = np.flatnonzero(whole.stopped_early)
    print(f"NEALS|placement|iters {whole.iters.tolist()}|repacks {info['repacks']}")
    assert 0 < len(stops) and len(set(whole.iters.tolist())) > 2
    for j in range(len(ks) * R):
        assert same(whole, packed, j), j
        assert same(whole, shards[0] if j < 11 else shards[1], j, 0 if j < 11 else 11), j
        assert same(whole, alone[j], j, j), j


# ---- 4. badly scaled Gram -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", [2.0 ** -40, 2.0 ** 30])
def test_badly_scaled_gram(scale):
    """One column of W0 times 2^-40, or times 2^30: cond(W0^T W0) grows by 2^80 / 2^60 from scaling alone.  An LU solve
    (what the kernels do) commutes with such a scaling up to the pivot order; a product with an explicit inverse of the
    Gram matrix does not.  FIXED 2, held to the bound of test_one_update_every_form."""
    from nmfconsensus_amd.nmf import Engine
    A, jk, W0, _ = case2(300, 70)
    W0 = [w.copy() for w in W0[:5]]   # k = 2..6
    for w in W0:
        w[:, 1] *= scale
    with Engine(A) as eng:
        r = eng.run(KS2, 1, maxiter=2, stop_rule=FIXED, W_init=W0, want_factors=True, neals=True, want_counts=False)
    assert not r.neals_status.any()
    for j, w0 in enumerate(W0):
        ld = nr.neals(A, w0, 2, fixed=True)
        yard = dist_wh(nr.neals(A, w0, 2, fixed=True, dtype=np.float64), ld)
        d = dist_wh(dict(W=r.W[j], H=r.H[j]), ld)
        print(f"NEALS|scaled|scale 2^{int(np.log2(scale))} k={jk[j]}|{d:.3e} of {bound_of(yard):.3e}")
        assert d <= bound_of(yard) and d <= TOL_REF, (j, d, yard)


# ---- 5. singular job ------------------------------------------------------------------------------------------------

def test_singular_job(capfd):
    """A W0 whose second column is exactly zero: the LU of W0^T W0 meets a zero pivot at iteration 1."""
    from nmfconsensus_amd import libnmf
    from nmfconsensus_amd.nmf import Engine
    A, _, W0all, _ = case2(300, 70)
    W0 = [w.copy() for w, k in zip(W0all, case2(300, 70)[1]) if k == 3][:4]
    Wz = W0[1]
    Wz[:, 1] = 0.0
    with Engine(A) as eng:
        r = eng.run([3], 4, maxiter=6, stop_rule=FIXED, W_init=W0, want_factors=True, neals=True)
        others = eng.run([3], 3, maxiter=6, stop_rule=FIXED, W_init=[W0[0], W0[2], W0[3]], want_factors=True, neals=True)
    assert r.neals_status.tolist() == [0, 1, 0, 0] and r.iters.tolist() == [6, 1, 6, 6]
    assert not r.stopped_early.any()
    assert np.array_equal(r.W[1], Wz) and not r.H[1].any()   # the factors of the last complete iteration: the inits
    assert r.labels[1].min() >= 1 and r.consensus is not None   # it still gets labels and is counted
    for a, b in ((0, 0), (2, 1), (3, 2)):
        assert np.array_equal(r.W[a], others.W[b]) and np.array_equal(r.H[a], others.H[b])
    h0 = np.random.default_rng(5).random((3, 70))
    capfd.readouterr()
    W, H, it, dn = libnmf.nmf_neals(A, Wz, h0, 6, 0.0, 0.0)
    err = capfd.readouterr().err
    assert dn == -1 and it == 1
    assert "zero pivot in the H solve at iteration 1" in err and "QR fallback is not implemented" in err
    assert np.array_equal(W, Wz) and np.array_equal(H, h0)


# ---- 6. drop-in and Python --------------------------------------------------------------------------------------------

def test_dropin_gives_the_engine_bits(golden):
    from nmfconsensus_amd import libnmf
    from nmfconsensus_amd.nmf import Engine
    A = golden["A_gct"]
    job = next(j for j in nr.golden_jobs()[2] if (j["mat"], j["k"], j["seed"], j["tolx"]) == (0, 3, 123, 1))
    W, H, it, dn = libnmf.nmf_neals(A, job["W0"], np.zeros((3, 40)), 2000, 1e-4, 1e-4)
    with Engine(A) as eng:
        r = eng.run([3], 1, maxiter=2000, stop_rule=TOLX_RULE, TolX=1e-4, TolFun=1e-4, W_init=[job["W0"]],
                    want_factors=True, want_residuals=True, neals=True)
    assert it == r.iters[0] == job["iters"]
    assert np.array_equal(W, r.W[0]) and np.array_equal(H, r.H[0])
    assert dn == libnmf.calculateNorm(A, W, H)[0]   # to the last bit
    # the engine's residual pass (want_residuals) sums the same m n squares in another order than calculateNorm's
    # pass, so the two figures of the same factors are held to each other at 4 ulps, not to equality (measured: 1 ulp);
    # the derived bound of the norm itself (tests/residual_bound.py) is an extra
    assert abs(r.dnorm[0] - dn) <= 4 * np.spacing(dn), (r.dnorm[0], dn)
    rb.check(dn, A, W, H, "nmf_neals return value")
    rb.check(r.dnorm[0], A, W, H, "engine residual")
    print(f"NEALS|dropin|iters {it}|dnorm {dn!r}|engine residual {r.dnorm[0]!r}|reference {job['dnorm']!r}")
    assert abs(dn - job["dnorm"]) <= 1e-9 * job["dnorm"]


def test_dropin_odd_count(golden):
    """FIXED 3 (TolX = TolFun = 0: no test can fire): the factors come back after an odd count, which the reference
    cannot do."""
    from nmfconsensus_amd import libnmf
    A = golden["A_gct"]
    job = next(j for j in nr.golden_jobs()[2] if (j["mat"], j["k"], j["seed"]) == (0, 3, 123))
    W, H, it, dn = libnmf.nmf_neals(A, job["W0"], np.zeros((3, 40)), 3, 0.0, 0.0)
    ld = nr.neals(A, job["W0"], 3, fixed=True)
    yard = dist_wh(nr.neals(A, job["W0"], 3, fixed=True, dtype=np.float64), ld)
    d = dist_wh(dict(W=W, H=H), ld)
    print(f"NEALS|dropin odd|{d:.3e} of {bound_of(yard):.3e}")
    assert it == 3 and d <= bound_of(yard)
    assert dn == libnmf.calculateNorm(A, W, H)[0]


def test_donmf_algorithm(golden):
    from nmfconsensus_amd import libnmf
    from nmfconsensus_amd.nmf import Engine, doNMF, release_doNMF_engine, runNMFinJobs
    A = golden["A_gct"]
    try:
        mu_default = doNMF(A, 3, 10000, seed=123)
        ne = doNMF(A, 3, 300, seed=123, tolerance=1e-4, algorithm="neals")
        mu = doNMF(A, 3, 10000, seed=123, algorithm="mu")
    finally:
        release_doNMF_engine()
    assert ne["status"] == 0 and 2 <= ne["iter"] <= 300 and ne["W"].shape == (1000, 3) and ne["H"].shape == (3, 40)
    # the same job through the engine: the init stream's W0 under the job seed, TolX = tolerance
    with Engine(A) as eng:
        r = eng.run([3], 1, maxiter=300, seed=123, stop_rule=1, TolX=1e-4, want_factors=True, want_residuals=True,
                    neals=True)
        assert eng._neals is False   # restored
    assert np.array_equal(ne["W"], r.W[0]) and np.array_equal(ne["H"], r.H[0]) and ne["iter"] == r.iters[0]
    # the job's residual against calculateNorm of its factors (what nmf_neals returns): 4 ulps, as in
    # test_dropin_gives_the_engine_bits (another summation order, so not equality); the derived bound is an extra
    dn = libnmf.calculateNorm(A, r.W[0], r.H[0])[0]
    print(f"NEALS|doNMF|residual {r.dnorm[0]!r}|calculateNorm {dn!r}")
    assert abs(r.dnorm[0] - dn) <= 4 * np.spacing(dn), (r.dnorm[0], dn)
    rb.check(r.dnorm[0], A, r.W[0], r.H[0], "doNMF neals job")
    # algorithm="mu" is the default and gives the bits it gave before
    assert mu["iter"] == mu_default["iter"] and "status" not in mu
    assert np.array_equal(mu["W"], mu_default["W"]) and np.array_equal(mu["H"], mu_default["H"])
    assert relfro(mu["H"], golden["refc_k3_H"]) <= TOL_REF   # the reference's nmf_mu from the same seed
    out = runNMFinJobs(A, [2, 3], 3, 50, 123, algorithm="neals", tolerance=1e-4)
    assert out["sweep"].neals_status is not None and not out["sweep"].neals_status.any()
    assert set(out["rho"]) == {"2", "3"}


def test_set_neals_excludes_euclid(golden):
    from nmfconsensus_amd import _lib
    from nmfconsensus_amd.nmf import Engine
    with Engine(golden["A_gct"]) as eng:
        eng.set_neals(True)
        with pytest.raises(ValueError, match="nmfc_engine_set_euclid failed"):
            eng.set_euclid(True)
        assert eng.L.nmfc_engine_neals_status(eng.h, None) == -1 and "not a NEALS run" in _lib.last_error()
        eng.set_neals(False)
        eng.set_euclid(True)
        with pytest.raises(ValueError, match="nmfc_engine_set_neals failed"):
            eng.set_neals(True)
        eng.set_euclid(False)
        mu = eng.run([3], 1, maxiter=20, stop_rule=FIXED, want_factors=True)
        assert mu.neals_status is None
        ne = eng.run([3], 1, maxiter=20, stop_rule=FIXED, want_factors=True, neals=True)
        again = eng.run([3], 1, maxiter=20, stop_rule=FIXED, want_factors=True)
    assert np.array_equal(mu.W[0], again.W[0]) and np.array_equal(mu.H[0], again.H[0])   # enable == 0 restores nmf_mu
    assert not np.array_equal(mu.W[0], ne.W[0])
