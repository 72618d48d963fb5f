"""Per-restart residual norms and the best factors per rank (nmfc_engine_set_residuals / _residuals / _best,
Engine.run(want_residuals=, want_best=)).

Every job's dnorm is held to the derived bound of tests/residual_bound.py against the long-double norm of the job's own
returned factors, on every path that fills the factor archive (solo kernels, k_small_mu, the MFMA sweep with and without
repacks, ragged tiles in both dimensions, caller inits on wide-range data).  Enabling residuals changes no other result
bit; a job's dnorm is byte-identical in any shard, group or batch; the best restart is the first argmin and its factors
are the ones want_factors returns.  Lines starting "RES|" print each figure beside its bound.
"""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest

import residual_bound as rb
import sched_fixture as sf
import widerange as wr

pytestmark = pytest.mark.gpu

FIXED, REF_COMPAT = 0, 1
DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int32)


@contextlib.contextmanager
def environ(env):
    """The engine knobs of `env` set while an engine is created and run, restored after."""
    saved = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def planted(m, n):
    from nmfconsensus_amd.synthetic import planted_matrix
    return planted_matrix(m, n)


def check_all(r, A, what):
    """Every job's dnorm within the bound of norm* from its own factors; returns the worst |error| / bound."""
    assert r.dnorm is not None and r.dnorm.dtype == np.float64 and r.dnorm.shape == (len(r.W),)
    assert np.all(np.isfinite(r.dnorm))
    return max(rb.check(r.dnorm[j], A, r.W[j], r.H[j], f"{what} job {r.job_begin + j} k={r.W[j].shape[1]}")
               for j in range(len(r.W)))


# ---- 1. value, every path ---------------------------------------------------------------------------------------------

def test_value_solo_kernels(golden):
    """(a) gct 1000 x 40, k = 2..5: each restart on a solo kernel."""
    from nmfconsensus_amd.nmf import Engine
    with Engine(golden["A_gct"]) as eng:
        r = eng.run([2, 3, 4, 5], 3, stop_rule=REF_COMPAT, want_residuals=True, want_factors=True)
        assert eng.last_run_info()["small"] == 1
        assert eng.L.nmfc_mu_solo_fits(1000, 40, 5) == 1
    check_all(r, golden["A_gct"], "solo gct")


def test_value_small_blocks(golden):
    """(b) gct, k = 9 and 16: k_small_mu blocks."""
    from nmfconsensus_amd.nmf import Engine
    with Engine(golden["A_gct"]) as eng:
        r = eng.run([9, 16], 3, stop_rule=REF_COMPAT, want_residuals=True, want_factors=True)
        assert eng.last_run_info()["small"] == 1
        assert eng.L.nmfc_mu_solo_fits(1000, 40, 9) == 0
    check_all(r, golden["A_gct"], "small gct")


@functools.lru_cache(maxsize=None)
def grid_c(R):
    """(c) 1100 x 72, k = 2, 7, 16, FIXED 30 on the MFMA path, with residuals, best and factors: (A, result)."""
    from nmfconsensus_amd.nmf import Engine
    A = sf.sched_A()
    with Engine(A) as eng:
        r = eng.run([2, 7, 16], R, maxiter=30, stop_rule=FIXED, want_best=True, want_factors=True)
        assert eng.last_run_info()["small"] == 0
    return A, r


def test_value_mfma():
    A, r = grid_c(3)
    assert np.all(r.iters == 30)
    check_all(r, A, "mfma 1100x72")


def test_value_ragged_tiles():
    """(d) 3001 x 150: 47 gene tiles, the last of 57 rows; two sample tiles, the last of 22 columns."""
    from nmfconsensus_amd.nmf import Engine
    A = planted(3001, 150)
    with Engine(A) as eng:
        r = eng.run([9], 2, maxiter=10, stop_rule=FIXED, want_residuals=True, want_factors=True)
    check_all(r, A, "mfma 3001x150")


@pytest.mark.parametrize("m,n", [(130, 17), (97, 33)])
def test_value_tiny_mfma(m, n):
    """(e) shapes below one tile in either dimension, taken off the small-shape kernels."""
    from nmfconsensus_amd.nmf import Engine
    A = planted(m, n)
    with environ({"NMFC_SMALL": "0"}), Engine(A) as eng:
        r = eng.run([3], 2, maxiter=10, stop_rule=FIXED, want_residuals=True, want_factors=True)
        assert eng.last_run_info()["small"] == 0
    check_all(r, A, f"mfma {m}x{n}")


def test_value_wide_range_caller_init():
    """(f) the wide-range A (a zero row, a zero column, twelve decades) from wide-range caller factors, two updates."""
    from nmfconsensus_amd.nmf import Engine
    m, n, ks, R = 1100, 72, (2, 7, 16), 3
    A = wr.wide_A(m, n, wr.SEED)
    jobs = [(ks[j % len(ks)], j // len(ks)) for j in range(len(ks) * R)]
    W0 = [wr.case("mu", m, n, k, q)[1] for k, q in jobs]
    H0 = [wr.case("mu", m, n, k, q)[2] for k, q in jobs]
    with Engine(A) as eng:
        r = eng.run(list(ks), R, maxiter=2, stop_rule=FIXED, W_init=W0, H_init=H0, want_residuals=True,
                    want_factors=True)
    assert np.all(r.dnorm > 0)
    check_all(r, A, "wide 1100x72")


# ---- 2. / 3. the schedule fixture: repacked archive; off means off ------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sched_runs():
    """The schedule fixture with residuals enabled and without, on one engine: (on, info_on, off, rc, message) with rc /
    message what nmfc_engine_residuals answers after the run that had them disabled."""
    from nmfconsensus_amd import _lib
    from nmfconsensus_amd.nmf import Engine
    with Engine(sf.sched_A()) as eng:
        on = eng.run(sf.KS, sf.R, maxiter=sf.MAXITER, seed=sf.SEED, stop_rule=REF_COMPAT, want_residuals=True,
                     want_factors=True)
        info = eng.last_run_info()
        off = eng.run(sf.KS, sf.R, maxiter=sf.MAXITER, seed=sf.SEED, stop_rule=REF_COMPAT, want_h=True)
        buf = np.full(sf.NJ, -7.0)
        rc = eng.L.nmfc_engine_residuals(eng.h, buf.ctypes.data_as(DP))
        msg = _lib.last_error()
        assert np.all(buf == -7.0)
    return on, info, off, rc, msg


def test_repacked_archive():
    on, info, _, _, _ = sched_runs()
    assert info["small"] == 0 and info["repacks"] >= 1
    assert np.array_equal(on.iters, sf.golden_sched()["iters"])
    check_all(on, sf.sched_A(), "sched")


def test_off_means_off():
    on, _, off, rc, msg = sched_runs()
    assert off.dnorm is None and off.best is None
    for name in ("iters", "stopped_early", "labels", "counts", "consensus"):
        assert np.array_equal(getattr(on, name), getattr(off, name)), name
    assert len(on.H) == len(off.H) == sf.NJ
    for j in range(sf.NJ):
        assert on.H[j].tobytes() == off.H[j].tobytes(), j
    assert rc == -1 and "residuals" in msg


# ---- 4. placement never changes a bit ---------------------------------------------------------------------------------

def test_placement_never_changes_a_bit():
    from nmfconsensus_amd.distributed import RestartGroups, merge_results
    from nmfconsensus_amd.nmf import Engine
    A, whole = grid_c(5)
    ks, R, kw = [2, 7, 16], 5, dict(maxiter=30, stop_rule=FIXED, want_residuals=True)
    want = whole.dnorm.tobytes()
    with Engine(A) as eng:
        parts = [eng.run(ks, R, job_begin=0, job_end=4, **kw), eng.run(ks, R, job_begin=4, **kw)]
        assert parts[0].W is None
        assert merge_results(parts).dnorm.tobytes() == want                 # two uneven shards, no factors asked for
        for j in (0, 7, 14):                                                # one-job shards
            one = eng.run(ks, R, job_begin=j, job_end=j + 1, **kw)
            assert one.dnorm.tobytes() == whole.dnorm[j:j + 1].tobytes(), j
        assert eng.run(ks, R, want_factors=True, **kw).dnorm.tobytes() == want
        assert eng.run(ks, R, **kw).dnorm.tobytes() == want
    with RestartGroups(A, device=0, groups=2) as grp:
        g = grp.run(ks, R, **kw)
        assert g.extras["groups"] == 2
        assert g.dnorm.tobytes() == want


# ---- 5. best ----------------------------------------------------------------------------------------------------------

def check_best(r, ks):
    nk = len(ks)
    assert sorted(r.best) == sorted(ks)
    for g, k in enumerate(ks):
        local = np.arange(r.job_end - r.job_begin)
        mine = local[(r.job_begin + local) % nk == g]
        first = int(mine[np.argmin(r.dnorm[mine])])
        b = r.best[k]
        assert b["job"] == r.job_begin + first, k
        assert b["dnorm"] == r.dnorm[first]
        if r.W is not None:
            assert b["W"].shape == r.W[first].shape and b["W"].tobytes(order="F") == r.W[first].tobytes(order="F"), k
            assert b["H"].shape == r.H[first].shape and b["H"].tobytes(order="F") == r.H[first].tobytes(order="F"), k


def test_best_is_first_argmin_with_its_factors():
    _, r = grid_c(5)
    check_best(r, [2, 7, 16])
    _, r3 = grid_c(3)
    check_best(r3, [2, 7, 16])


def test_best_of_merged_shards_and_absent_rank():
    from nmfconsensus_amd.distributed import merge_results
    from nmfconsensus_amd.nmf import Engine
    A, whole = grid_c(5)
    ks, R, kw = [2, 7, 16], 5, dict(maxiter=30, stop_rule=FIXED, want_best=True)
    m, n = A.shape
    with Engine(A) as eng:
        p1 = eng.run(ks, R, job_begin=2, job_end=15, **kw)
        p0 = eng.run(ks, R, job_begin=0, job_end=2, **kw)     # jobs 0, 1: no job of k = 16
        assert sorted(p0.best) == [2, 7]
        # the C ABI on that shard: -1 for k = 16, its W / H slots untouched, the others written
        job = np.full(3, 99, dtype=np.int32)
        dn = np.zeros(3)
        Wb = np.full(m * sum(ks), -3.0)
        Hb = np.full(n * sum(ks), -3.0)
        assert eng.L.nmfc_engine_best(eng.h, job.ctypes.data_as(IP), dn.ctypes.data_as(DP), Wb.ctypes.data_as(DP),
                                      Hb.ctypes.data_as(DP)) == 3
        assert job.tolist() == [0, 1, -1] and np.isnan(dn[2])
        assert np.all(Wb[m * 9:] == -3.0) and np.all(Hb[n * 9:] == -3.0)
        assert Wb[:m * 2].tobytes() == p0.best[2]["W"].tobytes(order="F")
        assert Hb[n * 2:n * 9].tobytes() == p0.best[7]["H"].tobytes(order="F")
    merged = merge_results([p0, p1])
    assert merged.dnorm.tobytes() == whole.dnorm.tobytes()
    for k in ks:
        assert merged.best[k]["job"] == whole.best[k]["job"], k
        assert merged.best[k]["dnorm"] == whole.best[k]["dnorm"]
        for f in ("W", "H"):
            assert merged.best[k][f].tobytes(order="F") == whole.best[k][f].tobytes(order="F"), (k, f)


def test_best_tie_takes_the_lower_job(golden):
    """Restarts 1 and 2 of k = 3 (jobs 0 and 2) start from identical caller factors: equal dnorm, and the lower job id
    is the best.  Restart 3 (job 4) cannot win: two of its three columns of W0 are zero, which the MU rule keeps zero, so
    it fits A with rank 1."""
    from nmfconsensus_amd.nmf import Engine
    A = golden["A_gct"]
    m, n = A.shape
    rng = np.random.default_rng(5)
    ks, R = [3, 9], 3
    jobs = [ks[j % 2] for j in range(2 * R)]
    W0 = [rng.uniform(0.1, 1.0, (m, k)) for k in jobs]
    H0 = [rng.uniform(0.1, 1.0, (k, n)) for k in jobs]
    W0[2], H0[2] = W0[0], H0[0]
    W0[4][:, 1:] = 0.0
    with Engine(A) as eng:
        r = eng.run(ks, R, maxiter=60, stop_rule=FIXED, W_init=W0, H_init=H0, want_best=True, want_factors=True)
    assert r.W[0].tobytes() == r.W[2].tobytes() and r.H[0].tobytes() == r.H[2].tobytes()
    assert r.dnorm[0] == r.dnorm[2]
    assert np.all(r.W[4][:, 1:] == 0.0) and r.dnorm[4] > r.dnorm[0]
    assert r.best[3]["job"] == 0
    check_best(r, ks)
    check_all(r, A, "tie gct")


# ---- 6. the C ABI directly --------------------------------------------------------------------------------------------

def test_c_abi_null_arguments(golden):
    from nmfconsensus_amd import _lib
    from nmfconsensus_amd.nmf import Engine
    L = _lib.lib()
    buf = np.zeros(8)
    ibuf = np.zeros(8, dtype=np.int32)
    L.nmfc_engine_set_residuals(None, 1)                        # ignored
    assert L.nmfc_engine_residuals(None, buf.ctypes.data_as(DP)) == -1 and _lib.last_error()
    assert L.nmfc_engine_best(None, ibuf.ctypes.data_as(IP), buf.ctypes.data_as(DP), None, None) == -1
    assert L.nmfc_engine_kernel_time(None, 8, None) == -1
    with Engine(golden["A_gct"]) as eng:
        assert L.nmfc_engine_residuals(eng.h, buf.ctypes.data_as(DP)) == -1    # no run yet
        assert L.nmfc_engine_best(eng.h, None, None, None, None) == -1
        r = eng.run([2, 3], 2, maxiter=5, stop_rule=FIXED, want_residuals=True)
        assert eng.kernel_time(8)[0] == 0                        # counted (one launch scope), not event-timed
        assert eng.kernel_flops(8) == sum((2 * k + 3) * 1000 * 40 for k in (2, 3, 2, 3))
        assert L.nmfc_engine_residuals(eng.h, None) == -1 and "NULL" in _lib.last_error()
        assert L.nmfc_engine_residuals(eng.h, buf.ctypes.data_as(DP)) == 4
        assert buf[:4].tobytes() == r.dnorm.tobytes() and np.all(buf[4:] == 0.0)
        # job ids and norms only: no factor leaves the device
        assert L.nmfc_engine_best(eng.h, ibuf.ctypes.data_as(IP), buf.ctypes.data_as(DP), None, None) == 2
        assert ibuf[0] in (0, 2) and ibuf[1] in (1, 3)
        assert buf[0] == r.dnorm[ibuf[0]] and buf[1] == r.dnorm[ibuf[1]]
        assert L.nmfc_engine_best(eng.h, None, None, None, None) == 2
        # the setting is restored after the call: the next plain run has none
        eng.run([2, 3], 2, maxiter=5, stop_rule=FIXED)
        assert L.nmfc_engine_residuals(eng.h, buf.ctypes.data_as(DP)) == -1


# ---- the reference-shaped driver --------------------------------------------------------------------------------------

def test_run_nmf_in_jobs_want_best(golden):
    """runNMFinJobs(..., want_best=True) adds 'best' and 'dnorm'; the default return is unchanged."""
    from nmfconsensus_amd.nmf import runNMFinJobs
    A = golden["A_gct"]
    plain = runNMFinJobs(A, [2, 3], 3, 10000, 123)
    out = runNMFinJobs(A, [2, 3], 3, 10000, 123, want_best=True)
    assert "best" not in plain and "dnorm" not in plain and plain["sweep"].dnorm is None
    assert sorted(set(out) - set(plain)) == ["best", "dnorm"]
    assert out["rho"] == plain["rho"] and np.array_equal(out["sweep"].labels, plain["sweep"].labels)
    assert out["dnorm"].shape == (6,)
    for g, k in enumerate([2, 3]):
        b = out["best"][k]
        assert b["job"] == g + 2 * int(np.argmin(out["dnorm"][g::2])) and b["dnorm"] == out["dnorm"][b["job"]]
        assert b["W"].shape == (1000, k) and b["H"].shape == (k, 40)
        rb.check(b["dnorm"], A, b["W"], b["H"], f"runNMFinJobs best k={k}")


def test_set_residuals_setting_survives_run(golden):
    """Engine.set_residuals(True) holds over run() calls that do not ask; want_residuals for one call leaves it off."""
    from nmfconsensus_amd.nmf import Engine
    with Engine(golden["A_gct"]) as eng:
        assert eng.run([2], 2, maxiter=3, stop_rule=FIXED).dnorm is None
        assert eng.run([2], 2, maxiter=3, stop_rule=FIXED, want_residuals=True).dnorm is not None
        assert eng.run([2], 2, maxiter=3, stop_rule=FIXED).dnorm is None
        eng.set_residuals(True)
        a = eng.run([2], 2, maxiter=3, stop_rule=FIXED)
        b = eng.run([2], 2, maxiter=3, stop_rule=FIXED, want_best=True)
        assert a.dnorm is not None and a.best is None and b.best is not None
        assert a.dnorm.tobytes() == b.dnorm.tobytes()
        assert eng.run([2], 2, maxiter=3, stop_rule=FIXED).dnorm is not None
