"""The BROAD script's Euclidean NMF() on the MFMA engine (nmfc_engine_set_euclid, Engine.run(euclid=),
brunet.NMF, brunet.nmfconsensus(error_function="euclidean")) against the numpy restatement of tests/euclid_ref.py.

1. values: FIXED T iterations against the long-double literal form, every W and H finite and >= 2^-52 (a NaN anywhere
   is the padded-gene-row bug); 2. the exact H rule on integer data, bit for bit; 3. the membership stop rule job for
   job against the Gram fp64 form; 4. the same bits under every placement (polls, repacks, shards, no narrow tail);
   5. the Python interface; 6. disabling restores the nmf_mu runs, and bad arguments are refused; 7. a restart that
   turns NaN (a zero column in its W0) stays alone: its neighbours in the batch and the next run on the engine keep
   their bits.  (Every element against a derived bound on wide-range data: tests/test_gpu_widerange.py.)
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


@pytest.mark.parametrize("m,n,k", [(130, 17, 3), (1100, 72, 5)])
def test_exact_h_rule_sees_a_fused_add(m, n, k):
    """The same with A in 0, 16, .., 112: most products H0 * q then lie above 2, where eps is half a unit in the last place
    and below, so the multiply and the add rounded as one (an FMA, what the compiler makes of the rule without its
    contract(off)) gives other bits than two roundings on part of the entries.  On test_exact_h_rule's own data the
    products lie below 2, where eps is a whole number of units and the two forms agree."""
    from nmfconsensus_amd.nmf import Engine
    rng = np.random.default_rng(m * 1000 + n + 1)
    A = np.asfortranarray(16.0 * rng.integers(0, 8, size=(m, n)).astype(np.float64))
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
        q = num / den
        want = H0[j] * q + er.EPS
        # H0 (3 bits) times q (53 bits) plus eps is exact in a 64-bit significand (the x87 long double that
        # tests/widerange.py also requires): one rounding to fp64 is then the FMA
        assert np.finfo(LD).eps <= 2.0 ** -63
        fused = (H0[j].astype(LD) * q.astype(LD) + LD(er.EPS)).astype(np.float64)
        told_apart += int((want != fused).sum())
        assert np.array_equal(r.H[j], want), (j, int((r.H[j] != want).sum()), int((r.H[j] == fused).sum()))
    print(f"EUC|exact H rule, A times 16|{m}x{n} k={k}|entries where a fused add gives other bits: {told_apart} of {R * k * n}")
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


# ---- 7. a poisoned restart stays alone --------------------------------------------------------------------------------
# The rule has no zero guard (nmfc.h: "IEEE results as R's"): a restart whose W0 has an all-zero column divides 0 by 0
# in the first H update.  R gives that restart NaN and nothing else; so must a batch that holds it, and so must the next
# run on the same engine.  The A h^T epilogue has a path of its own for a 16-column block that holds a non-finite W0,
# compiled into all five RULE_EUCLID forms, so the batches below reach each form:
#   narrow            200 x 60, k = 3, four restarts: twelve columns in one block, the 16-column narrow form;
#   200x60-tile*      k = 5, seven restarts, NMFC_NARROW=0: blocks of three restarts, [0 1 2] [3 4 5] [6] in one panel;
#                     the poisoned restart 4 is the middle one of block 1, with finite neighbours in its own block and in
#                     the blocks before and after it; the 64- and the 128-gene tile, n_pad - n = 4: no K-half skip;
#   1100x72-tile*     the same batch with n_pad - n = 24: the K-half skip, and nine gene tiles of 128.
# name: (m, n, k, R, the poisoned job, seed, environment, the A h^T form of last_run_info that must have run)
_WIDE = {"NMFC_NARROW": "0"}
POISON_CASES = {
    "narrow": (200, 60, 3, 4, 1, 67, {}, "ahtw_narrow"),
    "200x60-tile64": (200, 60, 5, 7, 4, 67, dict(_WIDE, NMFC_AHTW_TILE="64"), "ahtw_64"),
    "200x60-tile128": (200, 60, 5, 7, 4, 67, dict(_WIDE, NMFC_AHTW_TILE="128"), "ahtw_128"),
    "1100x72-tile64": (1100, 72, 5, 7, 4, 67, dict(_WIDE, NMFC_AHTW_TILE="64"), "ahtw_64"),
    "1100x72-tile128": (1100, 72, 5, 7, 4, 67, dict(_WIDE, NMFC_AHTW_TILE="128"), "ahtw_128"),
}
AHTW_FORMS = ("ahtw_narrow", "ahtw_64", "ahtw_128")


@functools.lru_cache(maxsize=None)
def poison_inits(name):
    """(W0 list, H0 list) of the healthy batch, and of the same batch with column 0 of the poisoned job's W0 set to 0.0."""
    m, n, k, R, bad, seed, _, _ = POISON_CASES[name]
    W0, H0 = zip(*(er.r_init(seed + i, m, n, k) for i in range(1, R + 1)))
    Wp = [w.copy(order="F") for w in W0]
    Wp[bad][:, 0] = 0.0
    return (list(W0), list(H0)), (Wp, list(H0))


def poison_run(eng, name, inits, **kw):
    """One batch of the case; asserts that every A h^T launch of the run took the form the case is there for."""
    _, _, k, R, _, _, _, form = POISON_CASES[name]
    r = eng.run([k], R, W_init=inits[0], H_init=inits[1], want_factors=True, euclid=kw.pop("euclid", DEFAULT), **kw)
    info = eng.last_run_info()
    assert info["small"] == 0 and info[form] >= r.iters.max() and all(info[f] == 0 for f in AHTW_FORMS if f != form), info
    return r


def assert_others_same(name, r, base, what):
    """Every job but the poisoned one: iteration count, early flag, labels, W and H bit-identical to the healthy batch."""
    R, bad = POISON_CASES[name][3], POISON_CASES[name][4]
    for j in range(R):
        if j == bad:
            continue
        assert r.iters[j] == base.iters[j] and r.stopped_early[j] == base.stopped_early[j], (what, j)
        assert np.array_equal(r.labels[j], base.labels[j]), (what, j)
        assert np.array_equal(r.W[j], base.W[j]) and np.array_equal(r.H[j], base.H[j]), \
            (what, j, int(np.isnan(r.W[j]).sum()), int(np.isnan(r.H[j]).sum()))


@pytest.mark.parametrize("name", list(POISON_CASES))
def test_poisoned_restart_fixed(name):
    """FIXED T = 1, 2, 3, with the residual pass on: the other jobs keep the healthy batch's bits (W, H, labels,
    dnorm); the poisoned job has the NaN pattern of the fp64 Gram form (T = 1: row 0 of H and all of W; from T = 2:
    everything), its finite entries at T = 1 within widerange.bound_u of that form, labels all 1 and dnorm NaN."""
    import widerange as wr
    from nmfconsensus_amd.nmf import Engine
    m, n, k, R, bad, _, env, _ = POISON_CASES[name]
    good, pois = poison_inits(name)
    V = er.planted(m, n)
    others = [j for j in range(R) if j != bad]
    with environ(env), Engine(V) as eng:
        for T in (1, 2, 3):
            base = poison_run(eng, name, good, maxiter=T, stop_rule=FIXED, want_residuals=True)
            r = poison_run(eng, name, pois, maxiter=T, stop_rule=FIXED, want_residuals=True)
            assert np.all(r.iters == T) and not r.stopped_early.any()
            assert np.all(np.isfinite(base.dnorm)) and all(np.isfinite(x).all() for x in base.W + base.H)
            with np.errstate(invalid="ignore", divide="ignore"):
                Wg, Hg, _, _ = er.run(V, pois[0][bad], pois[1][bad], T, form="gram", fixed=True)
            W, H = r.W[bad], r.H[bad]
            print(f"EUC|poison|{name}|FIXED T={T}|job {bad}: NaN in W {int(np.isnan(W).sum())} of {W.size}, in H "
                  f"{int(np.isnan(H).sum())} of {H.size}|other jobs: NaN in W "
                  f"{sum(int(np.isnan(r.W[j]).sum()) for j in others)}, in H {sum(int(np.isnan(r.H[j]).sum()) for j in others)}")
            assert np.array_equal(np.isnan(W), np.isnan(Wg)) and np.array_equal(np.isnan(H), np.isnan(Hg)), T
            assert not np.isinf(W).any() and not np.isinf(H).any()
            if T == 1:
                assert np.isnan(W).all() and np.isnan(H[0]).all() and np.isfinite(H[1:]).all()
                bh, _ = wr.bound_u(m, n, k, 1)
                eh = wr.cw_check(H[1:], Hg[1:], bh, "the finite rows of the poisoned job's H")
                print(f"EUC|poison|{name}|FIXED T=1|finite rows of H {eh:.0f} u of {bh}")
            else:
                assert np.isnan(W).all() and np.isnan(H).all()
            assert np.all(r.labels[bad] == 1)
            assert_others_same(name, r, base, f"FIXED T={T}")
            assert np.isnan(r.dnorm[bad])
            for j in others:
                assert r.dnorm[j] == base.dnorm[j], (T, j, r.dnorm[j], base.dnorm[j])


@pytest.mark.parametrize("check_every", [4, 1])
@pytest.mark.parametrize("name", list(POISON_CASES))
def test_poisoned_restart_membership_rule(name, check_every):
    """stopconv = 2, stopfreq = 1, maxiter = 50: the poisoned job's class never leaves 1 and the first check counts as
    a change, so it stops at t = 3; its columns then sit dead and full of NaN beside the other jobs, which run on
    and end as in the healthy batch."""
    from nmfconsensus_amd.nmf import Engine
    m, n, _, _, bad, _, env, _ = POISON_CASES[name]
    good, pois = poison_inits(name)
    rule = dict(stopconv=2, stopfreq=1)
    with environ(env), Engine(er.planted(m, n)) as eng:
        base = poison_run(eng, name, good, maxiter=50, euclid=rule, check_every=check_every)
        r = poison_run(eng, name, pois, maxiter=50, euclid=rule, check_every=check_every)
    print(f"EUC|poison|{name}|membership check_every={check_every}|iters {r.iters.tolist()} (healthy {base.iters.tolist()})|"
          f"early {r.stopped_early.tolist()}")
    assert r.iters[bad] == 3 and r.stopped_early[bad] == 1 and np.all(r.labels[bad] == 1)
    assert base.iters.max() > 3 + check_every     # the other jobs ran on beside the dead columns
    assert all(np.isfinite(x).all() for x in base.W + base.H)
    assert_others_same(name, r, base, f"membership rule, check_every={check_every}")


@pytest.mark.parametrize("name", list(POISON_CASES))
def test_engine_clean_after_poisoned_runs(name):
    """After the poisoned runs a healthy run on the same engine gives the bits of a fresh engine: nothing non-finite
    stays behind in padding, dead columns or the archive.  The same batch, and one of other ranks laid over them."""
    from nmfconsensus_amd.nmf import Engine
    m, n, _, _, _, seed, env, _ = POISON_CASES[name]
    good, pois = poison_inits(name)
    V = er.planted(m, n)

    def healthy(eng):
        return (poison_run(eng, name, good, maxiter=2, stop_rule=FIXED, want_residuals=True),
                eng.run([2, 5], 3, maxiter=2, seed=seed, stop_rule=FIXED, init_stream=INIT_R_RUNIF, want_factors=True,
                        want_residuals=True, euclid=DEFAULT))

    with environ(env), Engine(V) as eng:
        fresh = healthy(eng)
    with environ(env), Engine(V) as eng:
        for T in (1, 2, 3):
            poison_run(eng, name, pois, maxiter=T, stop_rule=FIXED, want_residuals=True)
        poison_run(eng, name, pois, maxiter=50, euclid=dict(stopconv=2, stopfreq=1))
        after = healthy(eng)
    for a, f in zip(after, fresh):
        assert np.array_equal(a.iters, f.iters) and np.array_equal(a.labels, f.labels)
        assert np.array_equal(a.dnorm, f.dnorm) and np.all(np.isfinite(a.dnorm))
        assert np.array_equal(a.counts, f.counts)
        for j in range(len(a.W)):
            assert np.array_equal(a.W[j], f.W[j]) and np.array_equal(a.H[j], f.H[j]), j
