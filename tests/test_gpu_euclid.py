"""The BROAD script's Euclidean NMF() on the MFMA engine (nmfc_engine_set_euclid, Engine.run(euclid=),
brunet.NMF, brunet.nmfconsensus(error_function="euclidean")) against the numpy restatement of tests/euclid_ref.py.

1. values: FIXED T iterations against the long-double literal form, every W and H finite and >= 2^-52 (a NaN anywhere
   is the padded-gene-row bug); 2. the exact H rule on integer data, bit for bit; 3. the membership stop rule job for
   job against the Gram fp64 form; 4. the same bits under every placement (polls, repacks, shards, no narrow tail);
   5. the Python interface; 6. disabling restores the nmf_mu runs, and bad arguments are refused.
Lines starting "EUC|" print each figure before it is asserted.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

import euclid_ref as er
import residual_bound as rb
import sched_fixture as sf
from conftest import relfro

pytestmark = pytest.mark.gpu

FIXED, REF_COMPAT, ARGMAX_STABLE, TOLX = 0, 1, 2, 3
INIT_R_RUNIF = 1
TOL = 1e-9          # the project's standing W / H tolerance (relative Frobenius error)
LD = np.longdouble
DEFAULT = dict(stopconv=40, stopfreq=10)


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


def engine_jobs(ks, R):
    """(k, restart i) of the engine's job order: k fastest."""
    return [(ks[j % len(ks)], j // len(ks) + 1) for j in range(len(ks) * R)]


# ---- 1. values --------------------------------------------------------------------------------------------------------

VALUE_CASES = {
    # name: (m, n, ks, R, seed, Ts)
    "97x33": (97, 33, [3], 1, 11, (1, 2, 30)),
    "130x17": (130, 17, [2, 5], 1, 23, (1, 2, 30)),
    "1100x72": (1100, 72, [2, 7, 16], 3, 37, (1, 2, 30)),
    "3001x150": (3001, 150, [9], 2, 41, (10,)),   # ragged last gene tile and sample tile
}


@functools.lru_cache(maxsize=None)
def value_reference(name):
    """{(k, i): {T: (W, H)}} in long double, the literal form, computed once per case."""
    m, n, ks, R, seed, Ts = VALUE_CASES[name]
    V = er.planted(m, n)
    out = {}
    for k, i in engine_jobs(ks, R):
        W0, H0 = er.r_init(seed + i, m, n, k)
        keep = {T: None for T in Ts}
        er.run(V, W0, H0, max(Ts), form="literal", dtype=LD, fixed=True, keep=keep)
        out[(k, i)] = keep
    return out


@pytest.mark.parametrize("name", list(VALUE_CASES))
def test_values(name):
    from nmfconsensus_amd.nmf import Engine
    m, n, ks, R, seed, Ts = VALUE_CASES[name]
    ref = value_reference(name)
    with Engine(er.planted(m, n)) as eng:
        for T in Ts:
            r = eng.run(ks, R, maxiter=T, seed=seed, stop_rule=FIXED, init_stream=INIT_R_RUNIF, want_factors=True,
                        want_counts=False, euclid=DEFAULT)
            assert eng.last_run_info()["small"] == 0
            assert np.all(r.iters == T) and not r.stopped_early.any()
            for j, (k, i) in enumerate(engine_jobs(ks, R)):
                W, H = r.W[j], r.H[j]
                Wl, Hl = ref[(k, i)][T]
                assert np.all(np.isfinite(W)) and np.all(np.isfinite(H)), (name, T, k, i, "NaN: a padded row was updated")
                assert W.min() >= er.EPS and H.min() >= er.EPS, (name, T, k, i, W.min(), H.min())
                ew = float(np.linalg.norm(W.astype(LD) - Wl) / np.linalg.norm(Wl))
                eh = float(np.linalg.norm(H.astype(LD) - Hl) / np.linalg.norm(Hl))
                print(f"EUC|values|{name}|T={T}|k={k} i={i}|W {ew:.3g}|H {eh:.3g}|bound {TOL:g}")
                assert ew <= TOL and eh <= TOL, (name, T, k, i, ew, eh)


# ---- 2. the exact H rule ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,k", [(130, 17, 3), (1100, 72, 5)])
def test_exact_h_rule(m, n, k):
    """A in 0..7, W0 and H0 in 1..4: every sum of the first H update is an exact integer (below 2^53) in any order, so
    H after T = 1 is H0 * (num / den) + eps from numpy bit for bit: the order divide, multiply, add and the eps."""
    from nmfconsensus_amd.nmf import Engine
    rng = np.random.default_rng(m * 1000 + n)
    A = np.asfortranarray(rng.integers(0, 8, size=(m, n)).astype(np.float64))
    R = 2
    W0 = [np.asfortranarray(rng.integers(1, 5, size=(m, k)).astype(np.float64)) for _ in range(R)]
    H0 = [np.asfortranarray(rng.integers(1, 5, size=(k, n)).astype(np.float64)) for _ in range(R)]
    with Engine(A) as eng:
        r = eng.run([k], R, maxiter=1, stop_rule=FIXED, W_init=W0, H_init=H0, want_factors=True, want_counts=False,
                    euclid=DEFAULT)
    told_apart = 0
    for j in range(R):
        num = W0[j].T @ A
        den = (W0[j].T @ W0[j]) @ H0[j]
        assert num.max() < 2.0 ** 53 and den.max() < 2.0 ** 53
        want = H0[j] * (num / den) + er.EPS
        assert np.array_equal(r.H[j], want), (j, np.abs(r.H[j] - want).max())
        told_apart += int((want != (H0[j] * num) / den + er.EPS).sum()) + int((want != H0[j] * (num / den)).sum())
        assert np.all(np.isfinite(r.W[j])) and r.W[j].min() >= er.EPS
    # multiply-then-divide, or no eps, gives other bits on this data: the comparison can tell the orders apart
    assert told_apart > 0


# ---- 3. the stop rule -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(er.STOP_SHAPES))
@pytest.mark.parametrize("setting", er.STOP_SETTINGS)
def test_stop_rule(shape, setting):
    from nmfconsensus_amd.nmf import Engine
    m, n = shape
    ref = er.stop_reference(shape, setting, "gram")
    with Engine(er.planted(m, n)) as eng:
        r = eng.run(er.STOP_KS, er.STOP_R, maxiter=er.STOP_MAXITER, seed=er.STOP_SHAPES[shape], init_stream=INIT_R_RUNIF,
                    want_counts=False, euclid=dict(stopconv=setting[0], stopfreq=setting[1]))
        assert eng.last_run_info()["small"] == 0
    bad = []
    for j, (k, i) in enumerate(engine_jobs(er.STOP_KS, er.STOP_R)):
        t, early, labels = ref[(k, i)]
        same = r.iters[j] == t and r.stopped_early[j] == early and np.array_equal(r.labels[j], labels)
        print(f"EUC|stop|{shape}|{setting}|k={k} i={i}|iters {r.iters[j]} vs {t}|early {r.stopped_early[j]} vs {early}|"
              f"labels differ {int((r.labels[j] != labels).sum())}")
        if not same and (shape, setting, k, i) not in er.STOP_EXCLUDED:
            bad.append((k, i, int(r.iters[j]), t))
    assert not bad, bad


def test_maxiter_below_first_possible_stop():
    """stopconv 40 / stopfreq 10 cannot stop before t = 410: maxiter = 400 runs them all, no early flag; and the rule
    firing exactly at maxiter still sets it."""
    from nmfconsensus_amd.nmf import Engine
    shape = (1000, 40)
    ref = er.stop_reference(shape, (40, 10), "gram")
    with Engine(er.planted(*shape)) as eng:
        r = eng.run(er.STOP_KS, er.STOP_R, maxiter=400, seed=er.STOP_SHAPES[shape], init_stream=INIT_R_RUNIF,
                    want_counts=False, euclid=DEFAULT)
        assert np.all(r.iters == 400) and not r.stopped_early.any()
        tmin = min(v[0] for v in ref.values())
        r = eng.run(er.STOP_KS, er.STOP_R, maxiter=tmin, seed=er.STOP_SHAPES[shape], init_stream=INIT_R_RUNIF,
                    want_counts=False, euclid=DEFAULT)
    assert np.all(r.iters == tmin)
    want = [int(ref[(k, i)][0] == tmin) for k, i in engine_jobs(er.STOP_KS, er.STOP_R)]
    assert r.stopped_early.tolist() == want and sum(want) >= 1


# ---- 4. placement -----------------------------------------------------------------------------------------------------

def sched_sweep(env=None, **kw):
    from nmfconsensus_amd.nmf import Engine
    with environ({k: str(v) for k, v in (env or {}).items()}):
        with Engine(sf.sched_A()) as eng:
            r = eng.run(sf.KS, sf.R, maxiter=2000, seed=sf.SEED, init_stream=INIT_R_RUNIF, want_factors=True,
                        euclid=DEFAULT, **kw)
            return r, eng.last_run_info()


@functools.lru_cache(maxsize=None)
def sched_base():
    return sched_sweep()


def assert_same_bits(r, base, what, offset=0):
    for j in range(len(r.iters)):
        b = offset + j
        assert r.iters[j] == base.iters[b] and r.stopped_early[j] == base.stopped_early[b], (what, b)
        assert np.array_equal(r.labels[j], base.labels[b]), (what, b)
        assert np.array_equal(r.W[j], base.W[b]) and np.array_equal(r.H[j], base.H[b]), (what, b)


def test_placement_default_schedule():
    r, info = sched_base()
    print(f"EUC|placement|default|{info}|iters {r.iters.min()}..{r.iters.max()}")
    assert info["small"] == 0 and info["repacks"] >= 1 and info["ahtw_narrow"] >= 1
    assert r.stopped_early.any() and r.iters.min() >= 410   # (some k = 9, 10 restarts run to the cap of 2000)
    for j in range(sf.NJ):
        assert np.all(np.isfinite(r.W[j])) and np.all(np.isfinite(r.H[j])) and r.W[j].min() >= er.EPS


@pytest.mark.parametrize("name,env,kw", [
    ("check_every=1", {}, dict(check_every=1)),
    ("check_every=16", {}, dict(check_every=16)),
    ("repack_div=1", {"NMFC_REPACK_DIV": 1}, {}),
    ("repack_div=1000", {"NMFC_REPACK_DIV": 1000}, {}),
    ("narrow=0", {"NMFC_NARROW": 0}, {}),
])
def test_placement_bit_identical(name, env, kw):
    base, _ = sched_base()
    r, info = sched_sweep(env, **kw)
    print(f"EUC|placement|{name}|{info}")
    assert info["small"] == 0
    if name == "narrow=0":
        assert info["ahtw_narrow"] == 0 and info["wta_narrow"] == 0
    assert_same_bits(r, base, name)


def test_placement_full_load_tile():
    """The 128-gene A h^T tile (the full-load form, here with the K-half skip: n_pad - n = 24) forced on the same
    sweep."""
    base, _ = sched_base()
    r, info = sched_sweep({"NMFC_AHTW_TILE": 128})
    print(f"EUC|placement|ahtw_tile=128|{info}")
    assert info["ahtw_128"] >= 1 and info["ahtw_64"] == 0
    assert_same_bits(r, base, "ahtw_tile=128")


def test_ahtw_forms_without_k_half_skip():
    """n_pad - n = 4 < 8: the 64- and the 128-gene A h^T tiles without the K-half skip, against the long-double literal
    form and each other (200 x 60: ragged last gene tile)."""
    from nmfconsensus_amd.nmf import Engine
    m, n, k, R, seed, T = 200, 60, 4, 2, 53, 10
    V = er.planted(m, n)
    got = {}
    for tile in (64, 128):
        with environ({"NMFC_AHTW_TILE": str(tile), "NMFC_NARROW": "0"}):
            with Engine(V) as eng:
                got[tile] = eng.run([k], R, maxiter=T, seed=seed, stop_rule=FIXED, init_stream=INIT_R_RUNIF,
                                    want_factors=True, want_counts=False, euclid=DEFAULT)
                info = eng.last_run_info()
                assert info["small"] == 0 and info[f"ahtw_{tile}"] == T, info
    for i in range(1, R + 1):
        W0, H0 = er.r_init(seed + i, m, n, k)
        Wl, Hl, _, _ = er.run(V, W0, H0, T, form="literal", dtype=LD, fixed=True)
        for tile in (64, 128):
            W, H = got[tile].W[i - 1], got[tile].H[i - 1]
            assert np.all(np.isfinite(W)) and np.all(np.isfinite(H)) and W.min() >= er.EPS and H.min() >= er.EPS
            ew = float(np.linalg.norm(W.astype(LD) - Wl) / np.linalg.norm(Wl))
            eh = float(np.linalg.norm(H.astype(LD) - Hl) / np.linalg.norm(Hl))
            print(f"EUC|values|200x60 tile {tile}|T={T}|k={k} i={i}|W {ew:.3g}|H {eh:.3g}|bound {TOL:g}")
            assert ew <= TOL and eh <= TOL
        assert np.array_equal(got[64].W[i - 1], got[128].W[i - 1]) and np.array_equal(got[64].H[i - 1], got[128].H[i - 1])


def test_placement_two_shards():
    base, _ = sched_base()
    cut = 41   # inside a restart's row of ks
    for b, e in ((0, cut), (cut, sf.NJ)):
        r, info = sched_sweep(job_begin=b, job_end=e)
        assert info["small"] == 0
        assert_same_bits(r, base, f"shard [{b}, {e})", offset=b)


# ---- 5. the interface -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def consensus_run():
    from nmfconsensus_amd.brunet import nmfconsensus
    V = er.planted(1000, 40)
    return V, nmfconsensus(V, 2, 4, 5, 2000, error_function="euclidean", rseed=9000, stopconv=5, stopfreq=3,
                           want_best=True)


def test_interface_nmf_is_one_restart_of_the_sweep():
    from nmfconsensus_amd.brunet import NMF
    V, out = consensus_run()
    sw = out["sweep"]
    ks, R = [2, 3, 4], 5
    assert sw.labels.shape == (len(ks) * R, 40) and out["error"].shape == (len(ks), R)
    for g, k in enumerate(ks):
        for i in (1, 4):   # restart i of rseed 9000 runs set.seed(9000 + i)
            one = NMF(V, k, maxniter=2000, seed=9000 + i, stopconv=5, stopfreq=3, want_error=True)
            q = g * R + i - 1
            assert one["t"] == sw.iters[q] and np.array_equal(er.membership(one["H"]), sw.labels[q]), (k, i)
            assert one["error"] == out["error"][g, i - 1], (k, i)
        # the best restart's factors are the ones NMF() gives from that restart's seed, bit for bit
        b = out["best"][k]
        one = NMF(V, k, maxniter=2000, seed=9000 + b["restart"] + 1, stopconv=5, stopfreq=3)
        assert np.array_equal(one["W"], b["W"]) and np.array_equal(one["H"], b["H"]), k


def test_interface_consensus_error_and_best():
    V, out = consensus_run()
    sw = out["sweep"]
    ks, R, (m, n) = [2, 3, 4], 5, V.shape
    L = sw.labels.reshape(len(ks), R, n)
    for g, k in enumerate(ks):
        C = np.zeros((n, n))
        for i in range(R):
            C += L[g, i][:, None] == L[g, i][None, :]
        assert np.array_equal(out["consensus"][str(k)], C / R), k
        b = out["best"][k]
        assert b["restart"] == int(np.argmin(out["error"][g])) and b["error"] == out["error"][g].min(), k   # first argmin
        # error.v on the returned factors: sqrt(sum((V - W H)^2)) / (m n) = norm* / sqrt(m n), within the residual
        # pass's derived bound plus 2 u for the division and its square root
        norm_s, bound = rb.norm_and_bound(V, b["W"], b["H"])
        want = norm_s / np.sqrt(LD(m) * LD(n))
        err = abs(LD(b["error"]) - want)
        allow = (bound + 2 * LD(2.0 ** -53) * norm_s) / np.sqrt(LD(m) * LD(n))
        print(f"EUC|error|k={k}|{b['error']:.17g}|error {float(err):.3g}|bound {float(allow):.3g}")
        assert err <= allow, k
    assert set(out) >= {"rho", "consensus", "membership", "order", "sweep", "error", "best"}


def test_interface_refusals():
    from nmfconsensus_amd.brunet import nmfconsensus
    V = er.planted(97, 33)
    with pytest.raises(ValueError):
        nmfconsensus(V, 2, 3, 2, 10, error_function="euclidean", want_divergence=True)
    with pytest.raises(ValueError):
        nmfconsensus(V, 2, 3, 2, 10, error_function="manhattan")


# ---- 6. off means off -------------------------------------------------------------------------------------------------

def test_off_means_off(golden):
    from nmfconsensus_amd.nmf import Engine
    ks, R = [int(x) for x in golden["c1_ks"]], int(golden["c1_R"])

    def c1(eng):
        return eng.run(ks, R, maxiter=10000, seed=int(golden["c1_seed"]), stop_rule=REF_COMPAT, want_factors=True)

    with Engine(golden["A_gct"]) as eng:
        before = c1(eng)
        assert eng.last_run_info()["small"] == 1
        eng.set_euclid(True, 5, 3)
        mid = eng.run(ks, 2, maxiter=50, seed=7, init_stream=INIT_R_RUNIF, want_factors=True)
        assert eng.last_run_info()["small"] == 0 and np.all(mid.iters >= 18)
        eng.set_euclid(False)
        after = c1(eng)
        assert eng.last_run_info()["small"] == 1
        # a per-call euclid= is gone after the call, too
        eng.run(ks, 1, maxiter=3, seed=7, euclid=DEFAULT, want_counts=False)
        again = c1(eng)
    for r in (after, again):
        assert np.array_equal(r.iters, golden["c1_iters"]) and np.array_equal(r.iters, before.iters)
        assert np.array_equal(r.labels, golden["c1_labels_argmax"]) and np.array_equal(r.counts, before.counts)
        for j in range(len(r.W)):
            assert np.array_equal(r.W[j], before.W[j]) and np.array_equal(r.H[j], before.H[j]), j


def test_bad_arguments():
    from nmfconsensus_amd import _lib
    from nmfconsensus_amd.nmf import Engine
    with Engine(er.planted(97, 33)) as eng:
        for stopconv, stopfreq in ((0, 10), (40, 0), (-1, -1)):
            assert eng.L.nmfc_engine_set_euclid(eng.h, 1, stopconv, stopfreq) == -1
            assert "nmfc_engine_set_euclid" in _lib.last_error()
            with pytest.raises(ValueError):
                eng.run([2], 1, maxiter=3, euclid=dict(stopconv=stopconv, stopfreq=stopfreq))
        assert eng.L.nmfc_engine_set_euclid(None, 1, 40, 10) == -1
        # a refused setting leaves the mode off: this is an nmf_mu run on the small-shape path
        eng.run([2], 1, maxiter=3, stop_rule=FIXED, want_counts=False)
        assert eng.last_run_info()["small"] == 1
