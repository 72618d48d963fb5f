"""A job's bits never depend on how the MU sweep was scheduled (plan_jobs / choose_tiles / repack / pack, engine.hip).

"Bits": a job's exit iteration, stop flag, labels, W and H.  "Scheduling": how many restarts are live, which W^T A or
A h^T tile the grid size picked, when the host polled, when it repacked the live restarts into fewer panels, whether
the tail ran on the narrow kernels.  One small sweep (sched_fixture.py: 1100 x 72, k = 2..10, R = 12; 108 jobs that
exit between ~400 and ~1300 iterations, so the packing shrinks from 12 panels to the narrow tail) runs the MFMA path's
poll / repack loop in well under a second; every variant below must reproduce the default schedule's run bit for bit,
and that run is pinned to the reference's own nmf_mu (golden_sched.npz) and to the oracle.  Engine.last_run_info() says
which schedule a run took, so no variant passes without having run what it names.
"""
import contextlib
import os

import numpy as np
import pytest

from conftest import relfro
from sched_fixture import KS, M, MAXITER, N, NJ, R, SEED, golden_sched, sched_A

pytestmark = pytest.mark.gpu

TOL = 1e-9   # north_star: per-restart W/H within 1e-9 relative Frobenius error
NK = len(KS)
# the schedule knobs nmfc_engine_create reads from the environment
KNOBS = ("NMFC_REPACK_DIV", "NMFC_NARROW", "NMFC_NARROW_MAXB", "NMFC_NARROW_LC", "NMFC_KCHUNK", "NMFC_WTA_TILE",
         "NMFC_AHTW_TILE")
WTA_WIDE = ("wta_sk", "wta_big", "wta_mid", "wta_small", "wta_tiny")
AHTW_WIDE = ("ahtw_128", "ahtw_64")


@contextlib.contextmanager
def knobs(env):
    """The engine's schedule knobs set to `env` (names without the NMFC_ prefix) and nothing else, restored after."""
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


def sweep(env=None, ks=KS, R=R, **kw):
    """One sweep on a fresh engine created under the knobs `env` -> (SweepResult, run info)."""
    from nmfconsensus_amd.nmf import Engine
    kw = {"maxiter": MAXITER, "seed": SEED, "want_factors": True, **kw}
    with knobs(env or {}), Engine(sched_A()) as eng:
        r = eng.run(ks, R, **kw)
        return r, eng.last_run_info()


class Runs:
    """The runs that several tests compare against, made once each."""

    def __init__(self):
        self.kept = {}

    def get(self, name, env=None, **kw):
        if name not in self.kept:
            self.kept[name] = sweep(env, **kw)
        return self.kept[name]

    def baseline(self):
        return self.get("baseline")


@pytest.fixture(scope="module")
def runs():
    c = Runs()
    yield c
    c.kept.clear()


@pytest.fixture(scope="module")
def oracle_jobs(oracle):
    """REF_COMPAT W, H and iterations from the oracle for the three jobs whose H the golden stores."""
    A = sched_A()
    out = {}
    for j in (int(x) for x in golden_sched()["H_jobs"]):
        W0, H0 = oracle.init_restart(SEED + j, M, N, KS[j % NK])
        out[j] = oracle.nmf_mu(A, W0, H0, MAXITER, 1)
    return out


def assert_same_bits(r, base, what, offset=0):
    """Every job of r equals job offset + i of base: iterations, stop flag, labels, W and H, bit for bit."""
    nj = len(r.iters)
    sl = slice(offset, offset + nj)
    for name in ("iters", "stopped_early"):
        a, b = getattr(r, name), getattr(base, name)[sl]
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (what, name, "first differing job", offset + int(bad[0]), int(a[bad[0]]), int(b[bad[0]]))
    bad = np.flatnonzero((r.labels != base.labels[sl]).any(axis=1))
    assert bad.size == 0, (what, "labels", "first differing job", offset + int(bad[0]))
    for i in range(nj):
        for name in ("W", "H"):
            a, b = getattr(r, name)[i], getattr(base, name)[offset + i]
            assert np.array_equal(a, b), (what, name, "first differing job", offset + i, "k", KS[(offset + i) % NK],
                                          "iterations", int(r.iters[i]), "relative difference", relfro(a, b))


def check_info(info, what, full=True):
    """What every MFMA-path run of this input reports."""
    assert info["small"] == 0 and info["repacks_skipped"] == 0 and info["wta_sk"] == 0, (what, info)
    # every enqueued iteration is one W^T A and one A h^T launch, each counted under exactly one form
    assert sum(info[k] for k in WTA_WIDE + ("wta_narrow",)) == info["iterations_enqueued"], (what, info)
    assert sum(info[k] for k in AHTW_WIDE + ("ahtw_narrow",)) == info["iterations_enqueued"], (what, info)
    assert info["wta_narrow"] == info["ahtw_narrow"], (what, info)
    if full:
        assert info["panels_first"] == 12, (what, info)
    assert 0 < info["panels_min"] <= info["panels_first"], (what, info)


def only_wide(info, wta, ahtw, what):
    """Of the full-width forms, only `wta` / `ahtw` ran."""
    for k in WTA_WIDE:
        assert (info[k] > 0) == (k == wta), (what, k, info)
    for k in AHTW_WIDE:
        assert (info[k] > 0) == (k == ahtw), (what, k, info)


# ---- a. the default schedule against the reference and the oracle ----

def test_baseline_vs_reference(runs, oracle_jobs):
    g = golden_sched()
    r, info = runs.baseline()
    assert np.array_equal(r.iters, g["iters"])
    assert np.array_equal(r.stopped_early, np.ones(NJ, dtype=np.int32))
    assert np.array_equal(r.labels, g["labels_argmax"])
    assert np.array_equal(r.counts, g["counts_argmax"])
    assert np.array_equal(r.consensus, g["counts_argmax"] / R)
    for q, j in enumerate(int(x) for x in g["H_jobs"]):
        assert relfro(r.H[j], g[f"H_{q}"]) < TOL, (j, relfro(r.H[j], g[f"H_{q}"]))
        Wo, Ho, ito = oracle_jobs[j]
        assert r.iters[j] == ito
        assert relfro(r.W[j], Wo) < TOL and relfro(r.H[j], Ho) < TOL, (j, relfro(r.W[j], Wo), relfro(r.H[j], Ho))
    check_info(info, "baseline")
    assert info["repacks"] >= 3 and info["panels_min"] < info["panels_first"], info
    assert info["wta_narrow"] > 0 and info["wta_tiny"] > 0, info
    assert info["polls"] * 4 >= info["iterations_enqueued"] >= int(g["iters"].max()), info


def test_baseline_r_order_labels(runs):
    # nmf.r:128's order()[1] labels: the same factors, the other label rule
    g = golden_sched()
    base, _ = runs.baseline()
    r, info = sweep(label_rule=1)
    assert np.array_equal(r.iters, g["iters"])
    assert np.array_equal(r.labels, g["labels_rorder"])
    assert np.array_equal(r.counts, g["counts_rorder"])
    for j in range(NJ):
        assert np.array_equal(r.W[j], base.W[j]) and np.array_equal(r.H[j], base.H[j]), j
    check_info(info, "r-order")


# ---- b. the schedule matrix under REF_COMPAT ----

SCHEDULES = {
    # check_every: when the host polls (and so when it may repack)
    "ce1": ({}, 1), "ce3": ({}, 3), "ce16": ({}, 16), "ce64": ({}, 64), "ce2000": ({}, 2000),
    # when it repacks
    "div1": ({"REPACK_DIV": 1}, 4), "div2": ({"REPACK_DIV": 2}, 4), "div1000": ({"REPACK_DIV": 1000}, 4),
    # the narrow tail
    "narrow0": ({"NARROW": 0}, 4), "maxb1": ({"NARROW_MAXB": 1}, 4), "maxb8": ({"NARROW_MAXB": 8}, 4),
    "lc0": ({"NARROW_LC": 0}, 4), "lc1": ({"NARROW_LC": 1}, 4),
    # crossed
    "ce1-div1000-big": ({"REPACK_DIV": 1000, "WTA_TILE": "big"}, 1),
    "ce64-div2-mid-64": ({"REPACK_DIV": 2, "WTA_TILE": "mid", "AHTW_TILE": "64"}, 64),
    "ce3-maxb8-small": ({"NARROW_MAXB": 8, "WTA_TILE": "small"}, 3),
}
# every forced tile pair, through the real repacks
for _w in ("big", "mid", "small", "tiny"):
    for _a in ("128", "64"):
        SCHEDULES[f"tile-{_w}-{_a}"] = ({"WTA_TILE": _w, "AHTW_TILE": _a}, 4)

INFOS = {}   # schedule name -> run info, for the assertions that compare two schedules


def run_schedule(runs, name):
    env, ce = SCHEDULES[name]
    base, _ = runs.baseline()
    r, info = sweep(env, check_every=ce)
    INFOS[name] = info
    assert_same_bits(r, base, name)
    check_info(info, name)
    return info


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_schedule_bit_identical(runs, name):
    _, binfo = runs.baseline()
    info = run_schedule(runs, name)
    env, ce = SCHEDULES[name]
    longest = int(golden_sched()["iters"].max())
    if ce == 1:
        assert info["polls"] == info["iterations_enqueued"], info
    if name == "ce2000":
        # every restart stops inside the first chunk and stays frozen in its columns through the rest of it
        assert longest < 2000 <= info["iterations_enqueued"] and info["repacks"] == 0 and info["polls"] <= 2, info
    if env.get("REPACK_DIV") == 1:
        assert info["repacks"] == 0 and info["panels_min"] == 12, info   # everything through archive_rest
        assert info["wta_narrow"] == 0, info
    if env.get("REPACK_DIV") == 1000:
        assert info["repacks"] > binfo["repacks"], (info, binfo)
    if env.get("REPACK_DIV") == 2:
        assert 0 < info["repacks"] <= binfo["repacks"], (info, binfo)
    if env.get("NARROW") == 0:
        assert info["wta_narrow"] == 0 and info["ahtw_narrow"] == 0, info
    if "NARROW_LC" in env or "NARROW_MAXB" in env:
        assert info["wta_narrow"] > 0, info
    if "WTA_TILE" in env:
        only_wide(info, "wta_" + env["WTA_TILE"], "ahtw_" + env["AHTW_TILE"] if "AHTW_TILE" in env else
                  next(k for k in AHTW_WIDE if info[k] > 0), name)
    if name.startswith("tile-"):
        assert info == {**binfo, **{k: info[k] for k in WTA_WIDE + AHTW_WIDE}}, (info, binfo)   # the real repacks
        assert info["repacks"] >= 3, info
    if "AHTW_TILE" in env:
        assert info["ahtw_" + env["AHTW_TILE"]] > 0, info


def test_narrow_maxb_widens_the_tail(runs):
    # the narrow form from 8 blocks on runs more of the sweep than the one-block form
    for name in ("maxb1", "maxb8"):
        if name not in INFOS:
            run_schedule(runs, name)
    _, binfo = runs.baseline()
    assert INFOS["maxb8"]["wta_narrow"] > binfo["wta_narrow"] > INFOS["maxb1"]["wta_narrow"] > 0, (INFOS["maxb8"], binfo,
                                                                                                  INFOS["maxb1"])


# ---- b'. the split-K family: NMFC_KCHUNK=512 sums W^T A in three gene chunks of 512, 512 and 128 ----

# jobs whose exit iteration or labels under KCHUNK=512 differ from the reference's by a near-tie in the argmax
# (at most 2 of the 108, each with its margin)
KCHUNK_EXCLUDED = {}

KCHUNK_SCHEDULES = {
    "k512-ce1": ({}, 1), "k512-ce64": ({}, 64), "k512-div1": ({"REPACK_DIV": 1}, 4),
    "k512-div1000": ({"REPACK_DIV": 1000}, 4), "k512-big": ({"WTA_TILE": "big"}, 4), "k512-tiny": ({"WTA_TILE": "tiny"}, 4),
}


def kchunk_base(runs):
    return runs.get("kchunk512", {"KCHUNK": 512})


def test_kchunk512_vs_reference(runs, oracle_jobs):
    g = golden_sched()
    r, info = kchunk_base(runs)
    base, _ = runs.baseline()
    check_info(info, "kchunk512")
    assert info["repacks"] >= 3 and info["wta_narrow"] > 0, info
    # another canonical summation order: some job's bits differ from the one-chunk run's (else the knob did nothing)
    assert any(not np.array_equal(r.W[j], base.W[j]) for j in range(NJ))
    assert len(KCHUNK_EXCLUDED) <= 2
    keep = np.array([j not in KCHUNK_EXCLUDED for j in range(NJ)])
    bad = np.flatnonzero((r.iters != g["iters"]) | (r.labels != g["labels_argmax"]).any(axis=1))
    print("KCHUNK=512 jobs differing from the reference:", [(int(j), int(r.iters[j]), int(g["iters"][j])) for j in bad])
    assert np.array_equal(r.iters[keep], g["iters"][keep]), [j for j in bad if keep[j]]
    assert np.array_equal(r.labels[keep], g["labels_argmax"][keep]), [j for j in bad if keep[j]]
    assert np.array_equal(r.stopped_early, np.ones(NJ, dtype=np.int32))
    for j, (Wo, Ho, ito) in oracle_jobs.items():
        assert j not in KCHUNK_EXCLUDED and r.iters[j] == ito
        assert relfro(r.W[j], Wo) < TOL and relfro(r.H[j], Ho) < TOL, (j, relfro(r.W[j], Wo), relfro(r.H[j], Ho))


@pytest.mark.parametrize("name", list(KCHUNK_SCHEDULES))
def test_kchunk512_schedule_bit_identical(runs, name):
    env, ce = KCHUNK_SCHEDULES[name]
    base, binfo = kchunk_base(runs)
    r, info = sweep({"KCHUNK": 512, **env}, check_every=ce)
    assert_same_bits(r, base, name)
    check_info(info, name)
    if ce == 1:
        assert info["polls"] == info["iterations_enqueued"], info
    if env.get("REPACK_DIV") == 1:
        assert info["repacks"] == 0, info
    if env.get("REPACK_DIV") == 1000:
        assert info["repacks"] > binfo["repacks"], (info, binfo)
    if "WTA_TILE" in env:
        only_wide(info, "wta_" + env["WTA_TILE"], next(k for k in AHTW_WIDE if info[k] > 0), name)


# ---- c. the other stop rules and iteration caps ----

RULES = {
    "argmax_stable": dict(stop_rule=2),
    "tolx": dict(stop_rule=3),
    "fixed37": dict(stop_rule=0, maxiter=37),   # odd, and no multiple of any check_every below
    "refcompat451": dict(maxiter=451),
}


@pytest.mark.parametrize("div", [1, 20])
@pytest.mark.parametrize("ce", [1, 4, 64])
@pytest.mark.parametrize("rule", list(RULES))
def test_stop_rule_schedule_bit_identical(runs, rule, ce, div):
    base, binfo = runs.get(rule, **RULES[rule])
    check_info(binfo, rule)
    r, info = sweep({"REPACK_DIV": div}, check_every=ce, **RULES[rule])
    what = f"{rule}-ce{ce}-div{div}"
    assert_same_bits(r, base, what)
    check_info(info, what)
    if ce == 1:
        assert info["polls"] == info["iterations_enqueued"], info
    if div == 1:
        assert info["repacks"] == 0, info
    elif rule != "fixed37" and ce <= 4:   # (at 64 the capped run's first poll that sees a stop is also its last)
        assert info["repacks"] >= 1, info
    if rule == "tolx":
        assert binfo["repacks"] >= 3, binfo   # Wsnap and k_wstat across repacks


@pytest.mark.parametrize("k", KS)
def test_argmax_stable_vs_oracle(runs, oracle, k):
    r, _ = runs.get("argmax_stable", **RULES["argmax_stable"])
    j = k - KS[0]   # the first restart of rank k
    W0, H0 = oracle.init_restart(SEED + j, M, N, k)
    Wo, Ho, ito = oracle.nmf_mu(sched_A(), W0, H0, MAXITER, 2)
    assert r.iters[j] == ito and r.stopped_early[j] == (ito < MAXITER)
    assert relfro(r.W[j], Wo) < TOL and relfro(r.H[j], Ho) < TOL, (relfro(r.W[j], Wo), relfro(r.H[j], Ho))


@pytest.mark.parametrize("k", KS)
def test_tolx_vs_oracle(runs, oracle, k):
    r, _ = runs.get("tolx", **RULES["tolx"])   # the default tolerances, TolX = TolFun = 1e-4
    j = k - KS[0]
    W0, H0 = oracle.init_restart(SEED + j, M, N, k)
    Wo, Ho, ito = oracle.nmf_mu_tol(sched_A(), W0, H0, MAXITER, 1e-4, 1e-4)
    assert r.iters[j] == ito and r.stopped_early[j] == (ito < MAXITER)
    assert relfro(r.W[j], Wo) < TOL and relfro(r.H[j], Ho) < TOL, (relfro(r.W[j], Wo), relfro(r.H[j], Ho))


def test_fixed37(runs, oracle):
    r, info = runs.get("fixed37", **RULES["fixed37"])
    assert np.array_equal(r.iters, np.full(NJ, 37, dtype=np.int32))
    assert np.array_equal(r.stopped_early, np.zeros(NJ, dtype=np.int32))
    assert info["iterations_enqueued"] == 37 and info["repacks"] == 0, info
    for j in (0, NK - 1, NJ - 1):
        W0, H0 = oracle.init_restart(SEED + j, M, N, KS[j % NK])
        Wo, Ho, _ = oracle.nmf_mu(sched_A(), W0, H0, 37, 0)
        assert relfro(r.W[j], Wo) < TOL and relfro(r.H[j], Ho) < TOL, j


def test_ref_compat_capped_at_451(runs):
    g_it = golden_sched()["iters"]
    early = g_it <= 451
    assert early.sum() >= 20 and (~early).sum() >= 20
    base, _ = runs.baseline()
    r, info = runs.get("refcompat451", **RULES["refcompat451"])
    fixed, _ = sweep(stop_rule=0, maxiter=451)
    assert info["iterations_enqueued"] == 451, info
    assert np.array_equal(r.iters, np.where(early, g_it, 451))
    assert np.array_equal(r.stopped_early, early.astype(np.int32))
    assert np.array_equal(fixed.iters, np.full(NJ, 451, dtype=np.int32))
    for j in range(NJ):
        want = base if early[j] else fixed
        assert np.array_equal(r.W[j], want.W[j]) and np.array_equal(r.H[j], want.H[j]), (j, bool(early[j]))
    late = np.flatnonzero(~early)
    assert np.array_equal(r.labels[late], fixed.labels[late])
    assert np.array_equal(r.labels[early], base.labels[early])


@pytest.mark.parametrize("maxiter", [0, 1])
def test_maxiter_0_and_1(oracle, maxiter):
    r, info = sweep(maxiter=maxiter)
    assert np.array_equal(r.iters, np.full(NJ, maxiter, dtype=np.int32))
    assert np.array_equal(r.stopped_early, np.zeros(NJ, dtype=np.int32))
    assert info["small"] == 0 and info["iterations_enqueued"] == maxiter and info["repacks"] == 0, info
    for j in range(NJ):
        k = KS[j % NK]
        W0, H0 = oracle.init_restart(SEED + j, M, N, k)
        if maxiter == 0:   # the init stream itself, bit for bit
            assert np.array_equal(r.W[j], W0) and np.array_equal(r.H[j], H0), j
        elif j % 13 == 0:
            Wo, Ho, _ = oracle.nmf_mu(sched_A(), W0, H0, 1, 0)
            assert relfro(r.W[j], Wo) < TOL and relfro(r.H[j], Ho) < TOL, j


# ---- d. batch and shard invariance on the MFMA path ----

def test_shards_bit_identical(runs):
    g = golden_sched()
    base, _ = runs.baseline()
    counts = 0
    its = []
    for b, e in ((0, 37), (37, 80), (80, 108)):
        r, info = sweep(job_begin=b, job_end=e)
        assert_same_bits(r, base, f"shard [{b}, {e})", offset=b)
        check_info(info, f"shard [{b}, {e})", full=False)
        assert info["panels_first"] < 12 and info["repacks"] >= 1, info
        counts = counts + r.counts
        its.append(r.iters)
    assert np.array_equal(np.concatenate(its), g["iters"])
    assert np.array_equal(counts, g["counts_argmax"])


def test_single_jobs_bit_identical(runs):
    from nmfconsensus_amd.nmf import Engine
    g = golden_sched()
    base, _ = runs.baseline()
    jobs = sorted({int(np.argmin(g["iters"])), int(np.argmax(g["iters"]))} | {NK * (1 + k % 3) + k - KS[0] for k in KS})
    assert {KS[j % NK] for j in jobs} == set(KS)
    with knobs({}), Engine(sched_A()) as eng:
        for j in jobs:
            r = eng.run(KS, R, maxiter=MAXITER, seed=SEED, want_factors=True, job_begin=j, job_end=j + 1)
            info = eng.last_run_info()
            assert_same_bits(r, base, f"job {j} alone", offset=j)
            check_info(info, f"job {j} alone", full=False)
            # one restart fits one 16-column block: narrow from the first iteration
            assert info["wta_narrow"] == info["iterations_enqueued"] >= g["iters"][j], info
            assert info["panels_first"] == 4 and info["repacks"] == 0, info


def test_restart_groups_bit_identical(runs):
    from nmfconsensus_amd.distributed import RestartGroups
    g = golden_sched()
    base, _ = runs.baseline()
    with knobs({}), RestartGroups(sched_A(), device=0, groups=2) as grp:
        r = grp.run(KS, R, maxiter=MAXITER, seed=SEED, want_factors=True)
        assert r.extras.get("groups") == 2
        for eng in grp.engines:
            check_info(eng.last_run_info(), "restart group", full=False)
    assert np.array_equal(r.counts, g["counts_argmax"])
    assert np.array_equal(r.consensus, g["counts_argmax"] / R)
    assert_same_bits(r, base, "two restart groups")


# ---- e. caller-provided init through the repacks ----

def test_caller_init_bit_identical(runs, oracle):
    base, binfo = runs.baseline()
    init = [oracle.init_restart(SEED + j, M, N, KS[j % NK]) for j in range(NJ)]
    r, info = sweep(W_init=[w for w, _ in init], H_init=[h for _, h in init])
    assert_same_bits(r, base, "caller init")
    assert np.array_equal(r.counts, base.counts)
    check_info(info, "caller init")
    assert info == binfo   # the same schedule, repacks included


# ---- f. a second run on an engine whose buffers hold an earlier, larger run ----

def test_engine_reuse_bit_identical(runs):
    from nmfconsensus_amd.nmf import Engine
    steps = [dict(ks=KS, R=R),
             dict(ks=KS, R=R, job_begin=80, job_end=108),
             dict(ks=[3, 10], R=2, stop_rule=3),
             dict(ks=[16], R=1, stop_rule=0, maxiter=5)]
    base, binfo = runs.baseline()
    with knobs({}), Engine(sched_A()) as eng:
        for q, st in enumerate(steps):
            kw = {"maxiter": MAXITER, "seed": SEED, "want_factors": True, **st}
            ks, Rq = kw.pop("ks"), kw.pop("R")
            r, info = eng.run(ks, Rq, **kw), eng.last_run_info()
            fresh, finfo = (base, binfo) if q == 0 else sweep(**st)
            assert np.array_equal(r.iters, fresh.iters), (q, r.iters, fresh.iters)
            assert np.array_equal(r.stopped_early, fresh.stopped_early), q
            assert np.array_equal(r.labels, fresh.labels), q
            assert np.array_equal(r.counts, fresh.counts), q
            for j in range(len(fresh.W)):
                assert np.array_equal(r.W[j], fresh.W[j]) and np.array_equal(r.H[j], fresh.H[j]), (q, j)
            assert info == finfo, (q, info, finfo)   # the info describes the last run only
            assert info["small"] == 0, info
    assert list(r.iters) == [5] and r.W[0].shape == (M, 16)
