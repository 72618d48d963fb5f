"""Per-restart KL divergence and the best factors per k on the Brunet path (nmfc_brunet_set_divergence / _divergence /
_best, BrunetEngine.run(want_divergence=, want_best=)).

Every job's D is held to the derived bound of tests/kl_bound.py against the long-double value of the job's own returned
factors: on the shapes of test_gpu_brunet*.py (one narrower than a wave's eight samples, ragged gene and sample tiles,
a zero row and a zero column), with one restart and with NMFC_BR_SMALL_B + 5, on an A with 30 % exact zeros, and on the
k = 2..10 sweep whose live list shrinks.  A job's D is byte-identical in any shard, batch and lane count; enabling it
changes no other result bit; the best restart is the first argmin and its factors are the ones want_factors returns.
Lines starting "KLD|" print each figure beside its bound, "KLD-LOG|" the device log's worst observed error in ulps.
"""
import ctypes
import functools

import numpy as np
import pytest

import kl_bound as kb

pytestmark = pytest.mark.gpu

NOSTOP = 10 ** 6   # stopconv no restart reaches: fixed iteration count
STOP = dict(seed=11, stopconv=3, stopfreq=5, maxiter=150)   # the stop rule of test_gpu_brunet_groups.py
DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int32)


@functools.lru_cache(maxsize=None)
def big_b():
    """NMFC_BR_SMALL_B + 5 of the built library: a batch that takes the tuned restart groups."""
    from nmfconsensus_amd import _lib
    f = _lib.lib().nmfc_build_tuning_brunet
    f.restype = ctypes.c_char_p
    got = dict(kv.split("=", 1) for kv in f().decode().split(";"))
    return int(got["NMFC_BR_SMALL_B"], 0) + 5


@functools.lru_cache(maxsize=None)
def shape_A(m, n):
    if (m, n) == (603, 300):   # the ragged matrix of test_gpu_brunet_groups.py: a zero row and a zero column
        A = np.asfortranarray(np.random.default_rng(603300).random((603, 300)) * 3.0)
        A[5, :] = 0.0
        A[:, 3] = 0.0
        return A
    A = np.asfortranarray(np.random.default_rng(m * 1000 + n).random((m, n)) * 3.0)   # test_gpu_brunet.py's
    A[0, :] = 0.0
    return A


def check_all(r, A, what):
    """Every job's D within the bound of D* from its own factors; returns the worst |error| / bound."""
    nk, B = len(r.ks), r.job_end - r.job_begin
    assert r.divergence is not None and r.divergence.dtype == np.float64 and r.divergence.shape == (nk, B)
    assert np.all(np.isfinite(r.divergence))
    worst = 0.0
    for ki, k in enumerate(r.ks):
        for b in range(B):
            j = ki * B + b
            worst = max(worst, kb.check(r.divergence[ki, b], A, r.W[j], r.H[j], f"{what} k={k} restart {r.job_begin + b}"))
    return worst


def device_log_ulps(eng, A, W, H):
    x = np.ascontiguousarray(kb.ratios(A, W, H))
    y = np.zeros_like(x)
    assert eng.L.nmfc_brunet_log_probe(eng.h, x.ctypes.data_as(DP), x.size, y.ctypes.data_as(DP)) == 0
    return kb.log_ulp_error(x, y)


# ---- 1. value ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,k", [(64, 5, 2), (333, 77, 7), (257, 256, 16), (603, 300, 2), (603, 300, 5),
                                   (603, 300, 10), (603, 300, 16)])
def test_value_one_restart_and_a_grouped_batch(m, n, k):
    """12 fixed iterations, B = 1 and B = NMFC_BR_SMALL_B + 5.  64 x 5 is narrower than a wave's eight samples (the
    rolled kernel); 333 x 77 and 603 x 300 end in a partly filled wave (77 = 9 * 8 + 5, 300 = 37 * 8 + 4) and a ragged
    gene tile; 257 rows leave 63 lanes of the last gene tile without a row."""
    from nmfconsensus_amd.brunet import BrunetEngine
    A = shape_A(m, n)
    with BrunetEngine(A) as eng:
        for B in (1, big_b()):
            r = eng.run([k], B, maxiter=12, seed=99, stopconv=NOSTOP, want_factors=True, want_divergence=True,
                        want_counts=False)
            assert np.all(r.iters == 12)
            assert r.best_restart is None and r.best_W is None
            check_all(r, A, f"{m}x{n} B={B}")
        ulps = device_log_ulps(eng, A, r.W[0], r.H[0])
    print(f"KLD-LOG|{m}x{n} k={k}|device log: worst {ulps:.3f} ulp over {m * n} ratios")
    assert ulps <= kb.L_LOG, f"the device log is {ulps:.3f} ulp off on this case: beyond the L = {kb.L_LOG} of the bound"


def test_value_with_exact_zeros():
    """30 % of A exactly 0: every such element contributes its p; D is finite and inside the bound."""
    from nmfconsensus_amd.brunet import BrunetEngine
    rng = np.random.default_rng(33377)
    A = np.asfortranarray(rng.random((333, 77)) * 3.0)
    A[rng.random(A.shape) < 0.3] = 0.0
    assert 0.25 < np.mean(A == 0.0) < 0.35
    with BrunetEngine(A) as eng:
        r = eng.run([7], 3, maxiter=12, seed=5, stopconv=NOSTOP, want_factors=True, want_divergence=True)
    assert np.all(np.isfinite(r.divergence)) and np.all(r.divergence > 0)
    check_all(r, A, "333x77 with zeros")


# ---- 2. / 3. / 4. the sweep whose live list shrinks --------------------------------------------------------------------

@pytest.fixture(scope="module")
def gct_brunet(golden):
    from nmfconsensus_amd.brunet import BrunetEngine
    eng = BrunetEngine(golden["A_gct"])
    yield eng
    eng.close()


KS = list(range(2, 11))


@pytest.fixture(scope="module")
def sweep(gct_brunet):
    """k = 2..10 with NMFC_BR_SMALL_B + 5 restarts each under the stop rule, on four lanes, with divergence, best and
    factors."""
    return gct_brunet.run(KS, big_b(), want_factors=True, want_best=True, lanes=4, **STOP)


def test_stop_rule_final_factors(sweep, golden):
    """Restarts stop at many different iterations (the live list shrinks through groups that are no multiple of RG): D
    is that of each job's final factors, those of restarts that stopped early included."""
    assert len(set(sweep.iters.tolist())) >= 10 and sweep.stopped_early.sum() >= len(KS) * (big_b() - 5)
    check_all(sweep, golden["A_gct"], "gct stop rule")


def test_placement_never_changes_a_bit(gct_brunet, sweep):
    B, nk = big_b(), len(KS)
    want = sweep.divergence.tobytes()
    kw = dict(want_divergence=True, **STOP)
    # two uneven shards, no factors asked for
    a = gct_brunet.run(KS, B, restart_end=16, **kw)
    b = gct_brunet.run(KS, B, restart_begin=16, **kw)
    assert a.W is None and a.divergence.shape == (nk, 16) and b.divergence.shape == (nk, B - 16)
    assert np.concatenate([a.divergence, b.divergence], axis=1).tobytes() == want
    # one-restart shards
    for i in (0, 15, 16, B - 1):
        one = gct_brunet.run(KS, B, restart_begin=i, restart_end=i + 1, **kw)
        assert one.divergence.tobytes() == np.ascontiguousarray(sweep.divergence[:, i:i + 1]).tobytes(), i
    # one lane and four, with and without the factors
    assert gct_brunet.run(KS, B, lanes=1, **kw).divergence.tobytes() == want
    assert gct_brunet.run(KS, B, lanes=4, **kw).divergence.tobytes() == want
    assert gct_brunet.run(KS, B, lanes=1, want_factors=True, **kw).divergence.tobytes() == want


def test_off_means_unchanged(gct_brunet, sweep):
    from nmfconsensus_amd import _lib
    B = big_b()
    off = gct_brunet.run(KS, B, want_factors=True, lanes=4, **STOP)
    assert off.divergence is None and off.best_restart is None and off.best_W is None
    for name in ("iters", "stopped_early", "labels", "counts", "consensus"):
        assert np.array_equal(getattr(sweep, name), getattr(off, name)), name
    for j in range(len(KS) * B):
        assert sweep.W[j].tobytes() == off.W[j].tobytes() and sweep.H[j].tobytes() == off.H[j].tobytes(), j
    buf = np.full(len(KS) * B, -7.0)
    ibuf = np.full(len(KS), 99, dtype=np.int32)
    assert gct_brunet.L.nmfc_brunet_divergence(gct_brunet.h, buf.ctypes.data_as(DP)) == -1
    assert "divergence" in _lib.last_error()
    assert gct_brunet.L.nmfc_brunet_best(gct_brunet.h, ibuf.ctypes.data_as(IP), buf.ctypes.data_as(DP), None, None) == -1
    assert np.all(buf == -7.0) and np.all(ibuf == 99)


# ---- 5. best ----------------------------------------------------------------------------------------------------------

def check_best(r):
    B = r.job_end - r.job_begin
    assert len(r.best_restart) == len(r.best_divergence) == len(r.best_W) == len(r.best_H) == len(r.ks)
    for ki, k in enumerate(r.ks):
        first = int(np.argmin(r.divergence[ki]))   # numpy's argmin is the first minimum
        assert r.best_restart[ki] == r.job_begin + first, k
        assert r.best_divergence[ki] == r.divergence[ki, first]
        W, H = r.W[ki * B + first], r.H[ki * B + first]
        assert r.best_W[ki].shape == W.shape and r.best_W[ki].tobytes(order="F") == W.tobytes(order="F"), k
        assert r.best_H[ki].shape == H.shape and r.best_H[ki].tobytes(order="F") == H.tobytes(order="F"), k


def test_best_is_first_argmin_with_its_factors(gct_brunet, sweep):
    check_best(sweep)
    assert len(set(sweep.best_restart)) > 1            # not the same restart for every k
    part = gct_brunet.run([3, 7], big_b(), restart_begin=20, restart_end=29, want_best=True, want_factors=True, **STOP)
    assert all(20 <= b < 29 for b in part.best_restart)
    check_best(part)
    for ki, k in enumerate((3, 7)):
        assert part.divergence[ki].tobytes() == np.ascontiguousarray(sweep.divergence[KS.index(k), 20:29]).tobytes()


def test_best_tie_takes_the_lower_restart(golden):
    """Four caller inits; the one that ends with the smallest D is then given to restarts 1 and 3 (0-based) and two of
    the others to restarts 0 and 2: equal D at 1 and 3, smaller than the rest, and the lower restart is the best."""
    from nmfconsensus_amd.brunet import BrunetEngine
    A = golden["A_gct"]
    m, n = A.shape
    rng = np.random.default_rng(5)
    R, k = 4, 3
    W0 = [rng.uniform(0.1, 1.0, (m, k)) for _ in range(R)]
    H0 = [rng.uniform(0.1, 1.0, (k, n)) for _ in range(R)]
    kw = dict(maxiter=40, stopconv=NOSTOP)
    with BrunetEngine(A) as eng:
        probe = eng.run([k], R, W_init=W0, H_init=H0, want_divergence=True, **kw)
        w = int(np.argmin(probe.divergence[0]))
        lose = [i for i in range(R) if i != w]
        order = [lose[0], w, lose[1], w]
        r = eng.run([k], R, W_init=[W0[i] for i in order], H_init=[H0[i] for i in order], want_best=True,
                    want_factors=True, **kw)
    assert r.divergence[0].tobytes() == probe.divergence[0][order].tobytes()   # a job's D does not depend on its slot
    assert r.W[1].tobytes() == r.W[3].tobytes() and r.H[1].tobytes() == r.H[3].tobytes()
    assert r.divergence[0, 1] == r.divergence[0, 3] < min(r.divergence[0, 0], r.divergence[0, 2])
    assert r.best_restart[0] == 1
    check_best(r)
    check_all(r, A, "tie gct")


def test_c_abi_and_empty_shard(golden):
    from nmfconsensus_amd import _lib
    from nmfconsensus_amd._lib import BrunetOpts, Result
    from nmfconsensus_amd.brunet import BrunetEngine
    L = _lib.lib()
    A = golden["A_gct"]
    m, n = A.shape
    buf = np.full(8, -7.0)
    ibuf = np.full(8, 99, dtype=np.int32)
    L.nmfc_brunet_set_divergence(None, 1)                        # ignored
    assert L.nmfc_brunet_divergence(None, buf.ctypes.data_as(DP)) == -1 and _lib.last_error()
    assert L.nmfc_brunet_best(None, ibuf.ctypes.data_as(IP), buf.ctypes.data_as(DP), None, None) == -1
    with BrunetEngine(A) as eng:
        assert L.nmfc_brunet_divergence(eng.h, buf.ctypes.data_as(DP)) == -1    # no run yet
        eng.set_timing(True)
        r = eng.run([2, 3], 2, maxiter=5, stopconv=NOSTOP, want_divergence=True, want_factors=True)
        cnt, ms, fl = eng.kernel_time(_lib.BK_DIV)
        assert cnt == 2 and ms > 0.0 and fl == sum((2 * k + 6 + 83) * m * n * 2 for k in (2, 3)) / 2
        assert eng.kernel_time(4)[0] == -1
        eng.set_timing(False)
        # the setting of one call is restored after it: the C functions answer for the last run, which had it on
        assert L.nmfc_brunet_divergence(eng.h, None) == -1 and "NULL" in _lib.last_error()
        assert L.nmfc_brunet_divergence(eng.h, buf.ctypes.data_as(DP)) == 4
        assert buf[:4].tobytes() == r.divergence.tobytes() and np.all(buf[4:] == -7.0)
        # restarts and values only: no factor leaves the device
        assert L.nmfc_brunet_best(eng.h, ibuf.ctypes.data_as(IP), buf.ctypes.data_as(DP), None, None) == 2
        assert ibuf[:2].tolist() == [int(np.argmin(r.divergence[g])) for g in (0, 1)] and np.all(ibuf[2:] == 99)
        assert buf[0] == r.divergence[0].min() and buf[1] == r.divergence[1].min()
        assert L.nmfc_brunet_best(eng.h, None, None, None, None) == 2
        Wb = np.full(m * 5, -3.0)
        Hb = np.full(n * 5, -3.0)
        assert L.nmfc_brunet_best(eng.h, None, None, Wb.ctypes.data_as(DP), Hb.ctypes.data_as(DP)) == 2
        for g, (wo, ho, k) in enumerate(((0, 0, 2), (2 * m, 2 * n, 3))):
            j = g * 2 + int(ibuf[g])
            assert Wb[wo:wo + m * k].tobytes() == r.W[j].tobytes(order="F"), g
            assert Hb[ho:ho + k * n].tobytes() == r.H[j].tobytes(order="F"), g
        # a shard without restarts: the run is refused as before, and the divergence calls answer -1 and write nothing
        eng.set_divergence(True)
        o = BrunetOpts()
        L.nmfc_brunet_default_opts(ctypes.byref(o))
        o.maxiter, o.restart_begin, o.restart_end = 5, 2, 2
        ks = np.array([2, 3], dtype=np.int32)
        res = Result()
        assert L.nmfc_brunet_run(eng.h, ks.ctypes.data_as(IP), 2, 2, ctypes.byref(o), None, None, ctypes.byref(res)) == -1
        assert "empty restart range" in _lib.last_error()
        buf[:] = -7.0
        ibuf[:] = 99
        Wb[:] = -3.0
        Hb[:] = -3.0
        assert L.nmfc_brunet_divergence(eng.h, buf.ctypes.data_as(DP)) == -1
        assert L.nmfc_brunet_best(eng.h, ibuf.ctypes.data_as(IP), buf.ctypes.data_as(DP), Wb.ctypes.data_as(DP),
                                  Hb.ctypes.data_as(DP)) == -1
        assert np.all(buf == -7.0) and np.all(ibuf == 99) and np.all(Wb == -3.0) and np.all(Hb == -3.0)
        eng.set_divergence(False)
        # a plain run afterwards has none
        eng.run([2], 2, maxiter=3, stopconv=NOSTOP)
        assert L.nmfc_brunet_divergence(eng.h, buf.ctypes.data_as(DP)) == -1


# ---- the script-shaped entry points -----------------------------------------------------------------------------------

def test_nmfconsensus_and_nmf_div_keywords(golden):
    from nmfconsensus_amd.brunet import NMF_div, nmfconsensus
    A = golden["A_gct"]
    plain = nmfconsensus(A, 2, 3, 4, 60)
    out = nmfconsensus(A, 2, 3, 4, 60, want_best=True)
    assert "best" not in plain and "divergence" not in plain and plain["sweep"].divergence is None
    assert sorted(set(out) - set(plain)) == ["best", "divergence"]
    assert out["rho"] == plain["rho"] and np.array_equal(out["sweep"].labels, plain["sweep"].labels)
    assert out["divergence"].shape == (2, 4)
    for g, k in enumerate((2, 3)):
        b = out["best"][k]
        assert b["restart"] == int(np.argmin(out["divergence"][g])) and b["divergence"] == out["divergence"][g].min()
        assert b["W"].shape == (1000, k) and b["H"].shape == (k, 40)
        kb.check(b["divergence"], A, b["W"], b["H"], f"nmfconsensus best k={k}")
    one = NMF_div(A, 3, maxniter=20, seed=42, stopconv=NOSTOP, want_divergence=True)
    assert "divergence" not in NMF_div(A, 3, maxniter=20, seed=42, stopconv=NOSTOP)
    kb.check(one["divergence"], A, one["W"], one["H"], "NMF_div k=3")
