"""The stream-K W^T A tile (k_wta2_sk) gives the bits of the one-item-per-workgroup tile (k_wta2) on every path it has.

k_wta2_sk runs #CU persistent workgroups: whole rounds of items first (D items, `pc < ndp`), then the remaining one to
two rounds' worth of stages split evenly, a split item's MFMA chains handed from its start piece to its continuation
through a slot and an agent-scope flag.  A continuation that does not see the flag within ~0.9 ms recomputes the whole
item from stage 0.  The design's claim is that none of this changes a bit; each test below runs three arms --
NMFC_WTA_SK=0 (k_wta2), NMFC_WTA_SK=1, and NMFC_WTA_SK=1 with NMFC_WTA_SK_NOWAIT=1 (the NOWAIT instantiations, in which
every continuation takes the recompute path) -- and compares W, H, iterations, stop flags and labels of every job with
np.array_equal.  Engine.last_run_info() proves per arm which kernel ran, so no arm passes by comparing k_wta2 with itself.

a. FIXED iterations on grids below two rounds of items (D = 0) and on grids of three rounds and more with one and with
   two whole rounds (D = #CU, D = 2 #CU: `pc < ndp` with pc = 0 and 1, off() / locate() with base > 0), the latter also
   with the XCD-contiguous round order; sk_plan() mirrors sk_grid_fits and the kernel's D so each case states its
   regime.  (The 2-panel tile at m = 4200, R = 160 holds 3.2 rounds, not fewer than two: its D = 0 grid is R = 80.)
b. Restarts that stop while every launch is still stream-K (never repacked, no narrow tail): partly live and wholly
   dead 4-panel groups (`if (!any) return` on both pieces of an item, live[] / need[]), and the default schedule.
   Stop rule: REF_COMPAT (stop_rule=1), chosen once from the NMFC_WTA_SK=0 arm on the planted 4200 x 500 matrix.
c. Two restart groups (two engines, each with its own #CU persistent workgroups of 144 KiB LDS) at a stream-K grid.
   Nothing observes whether the two groups' launches overlapped on the GPU, or whether any poll timed out: the test pins
   the results of the configuration in which a start piece may not be resident when its continuation polls, not the event.

The epoch case of (a) starts the launch counter (the hand-off flag value) at 2^32 - 3, so its six launches cross the
32-bit wrap: launch_wta_sk then zeroes the flags and restarts the count at 1 instead of using 0, the value of a slot
nobody has published.  The run info's sk_wraps == 1 (0 in every other case) shows that the wrap path ran; the arms show
that it keeps the bits.  It is no regression test: it could not
fail on the code before the fix either, because the hazard also needs a start piece that loses a race at that launch.
"""
import contextlib
import os

import numpy as np
import pytest

from conftest import relfro

pytestmark = pytest.mark.gpu

TOL = 1e-9   # north_star: per-restart W/H within 1e-9 relative Frobenius error
N = 500
KS = list(range(2, 11))
NK = len(KS)
SEED = 9
STOP_RULE = 1      # (b), (c): REF_COMPAT
MAXITER = 10000    # a cap above the longest exit (asserted)
# every knob nmfc_engine_create reads that a run here could depend on
KNOBS = ("NMFC_WTA_SK", "NMFC_WTA_SK_MID", "NMFC_WTA_SK_NOWAIT", "NMFC_WTA_SK_EPOCH0", "NMFC_WTA_LASTSUM",
         "NMFC_SK_DP_XCD", "NMFC_WTA_TILE", "NMFC_AHTW_TILE", "NMFC_REPACK_DIV", "NMFC_NARROW", "NMFC_NARROW_MAXB",
         "NMFC_NARROW_LC", "NMFC_KCHUNK", "NMFC_GRAM_MODEL")
WTA_OTHER = ("wta_narrow", "wta_big", "wta_mid", "wta_small", "wta_tiny")
ARMS = {"sk0": {"WTA_SK": 0}, "sk1": {"WTA_SK": 1}, "nowait": {"WTA_SK": 1, "WTA_SK_NOWAIT": 1}}


@contextlib.contextmanager
def knobs(env):
    """The engine's knobs set to `env` (names without the NMFC_ prefix) and nothing else, restored after."""
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


def ncu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- the host's packing and the kernel's split, mirrored so that each case can say which regime it is in ----

def packed_panels(ks, R):
    """(panels holding restarts, panels of the padded packing) of the first packing of the len(ks) * R jobs: pack() in
    engine.hip -- ranks descending, first fit into 16-column blocks, four blocks a panel, panels padded to four."""
    fill, first_open = [], 0
    for k in sorted((k for k in ks for _ in range(R)), reverse=True):
        b = first_open
        while b < len(fill) and fill[b] + k > 16:
            b += 1
        if b == len(fill):
            fill.append(0)
        fill[b] += k
        while first_open < len(fill) and fill[first_open] > 14:
            first_open += 1
    live = max(1, (len(fill) + 3) // 4)
    return live, (live + 3) // 4 * 4


def sk_plan(m, n, ks, R, tile, G):
    """sk_grid_fits (engine.hip) and k_wta2_sk's D (nmfc_kernels.hpp) for the first packing on G compute units."""
    m_pad = (m + 127) // 128 * 128
    kchunk = min(2048, m_pad)
    nsplit = (m_pad + kchunk - 1) // kchunk
    ntj = (n + 127) // 128
    live, padded = packed_panels(ks, R)
    ng = padded // 4 if tile == "big" else (live + 1) // 2
    ipc = ng * ntj
    nitems = ipc * nsplit
    nst_full, nst_last = kchunk // 16, (m_pad - (nsplit - 1) * kchunk) // 16
    nst_max = nst_full if nsplit > 1 else nst_last
    c_last = ipc * (nsplit - 1)

    def off(item):
        return item * nst_full if item <= c_last else c_last * nst_full + (item - c_last) * nst_last

    fits = ntj >= 4 and nitems >= G and off(nitems) >= G * nst_max
    D = max(0, (nitems // G - 1) * G)
    while D > 0 and off(nitems) - off(D) < G * nst_max:
        D -= G
    return dict(fits=fits, nitems=nitems, rounds=nitems / G, D=D, ndp=D // G, panels=padded, nsplit=nsplit)


def restarts_for_whole_rounds(m, tile, G):
    """The smallest even R whose grid holds at least three rounds of items of which the kernel runs two or more whole."""
    for R in range(100, 1200, 2):
        p = sk_plan(m, N, KS, R, tile, G)
        if p["fits"] and p["nitems"] // G >= 3 and p["ndp"] >= 2:
            return R
    raise AssertionError(("no R below 1200 gives two whole rounds", m, tile, G))


# ---- runs and comparisons ----

def run_engine(A, env, R, **kw):
    """One sweep on a fresh engine created under the knobs `env` -> (SweepResult, run info)."""
    from nmfconsensus_amd.nmf import Engine
    kw = {"seed": SEED, "want_factors": True, "want_counts": False, **kw}
    with knobs(env), Engine(A) as eng:
        r = eng.run(KS, R, **kw)
        return r, eng.last_run_info()


def assert_same_bits(r, base, what, offset=0):
    """Every job i of base equals job offset + i of r: iterations, stop flag, labels, W and H, bit for bit."""
    nj = len(base.iters)
    sl = slice(offset, offset + nj)
    for name in ("iters", "stopped_early"):
        a, b = getattr(r, name)[sl], getattr(base, name)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (what, name, "first differing job", offset + int(bad[0]), int(a[bad[0]]), int(b[bad[0]]),
                               "jobs differing", int(bad.size))
    bad = np.flatnonzero((r.labels[sl] != base.labels).any(axis=1))
    assert bad.size == 0, (what, "labels", "first differing job", offset + int(bad[0]), "jobs differing", int(bad.size))
    for i in range(nj):
        for name in ("W", "H"):
            a, b = getattr(r, name)[offset + i], getattr(base, name)[i]
            assert np.array_equal(a, b), (what, name, "first differing job", offset + i, "k", KS[(offset + i) % NK],
                                          "iterations", int(base.iters[i]), "relative difference", relfro(a, b))


def assert_stream_k_ran(info, arm, what, launches=None):
    """The run info of an arm: which W^T A kernel its launches were."""
    print(what, arm, info)
    assert info["small"] == 0, (what, arm, info)
    if arm == "sk0":
        assert info["wta_sk"] == 0 and info["wta_sk_nowait"] == 0, (what, arm, info)
        return
    if launches is not None:
        assert info["wta_sk"] == launches == info["iterations_enqueued"], (what, arm, info)
        assert all(info[k] == 0 for k in WTA_OTHER), (what, arm, info)
    assert info["wta_sk"] > 0, (what, arm, info)
    assert info["wta_sk_nowait"] == (info["wta_sk"] if arm == "nowait" else 0), (what, arm, info)


class Kept:
    """Inputs and NMFC_WTA_SK=0 runs that more than one case uses, made once; one run kept at a time (they are large)."""

    def __init__(self):
        self.A = {}
        self.key, self.run = None, None

    def random_A(self, m):
        if ("random", m) not in self.A:
            self.A[("random", m)] = np.asfortranarray(np.random.default_rng(m).random((m, N)) * 3.0)
        return self.A[("random", m)]

    def planted_A(self, m):
        from nmfconsensus_amd.synthetic import planted_matrix
        if ("planted", m) not in self.A:
            self.A[("planted", m)] = planted_matrix(m, N)
        return self.A[("planted", m)]

    def base(self, key, make):
        if self.key != key:
            self.key, self.run = None, None   # the previous one goes first
            self.key, self.run = key, make()
        return self.run


@pytest.fixture(scope="module")
def kept():
    c = Kept()
    yield c
    c.A.clear()
    c.key, c.run = None, None


# ---- a. FIXED iterations, three arms ----

T = 6
FIXED_CASES = {
    # name: (tile, m, R or None for "from the CU count", regime, knobs of the stream-K arms).  Regimes on 256 CUs:
    # lt2: fewer than two rounds of items, D = 0 (no whole rounds: every item in the split part);
    # ge3: three rounds or more and D > 0 (whole rounds run, base > 0); ge3x2: ... of which at least two whole
    # (pc = 1: item G + r, and the XCD-contiguous order's ndp xb + pc xc).
    # m = 4200: three gene chunks, the last 128 genes (8 stages) long; m = 2000: one chunk
    "big-4200-R160": ("big", 4200, 160, "lt2", {}),
    # the flag values 2^32 - 2 and 2^32 - 1, then the wrap (flags zeroed, 1), 2, 3, 4
    "big-4200-R160-epoch": ("big", 4200, 160, "lt2", {"WTA_SK_EPOCH0": 4294967293}),
    "big-2000-R310": ("big", 2000, 310, "lt2", {}),
    "mid-4200-R80": ("mid", 4200, 80, "lt2", {}),
    "mid-2000-R160": ("mid", 2000, 160, "lt2", {}),
    "mid-4200-R160": ("mid", 4200, 160, "ge3", {}),     # 828 two-panel items: 3.2 rounds, one of them whole
    "big-4200-rounds": ("big", 4200, None, "ge3x2", {}),
    "big-4200-rounds-xcd": ("big", 4200, None, "ge3x2", {"SK_DP_XCD": 1}),
    "mid-4200-rounds": ("mid", 4200, None, "ge3x2", {}),
}


@pytest.mark.parametrize("name", list(FIXED_CASES))
def test_fixed_iterations_three_arms(kept, oracle, name):
    tile, m, R, regime, extra = FIXED_CASES[name]
    G = ncu()
    if R is None:
        R = restarts_for_whole_rounds(m, tile, G)
    plan = sk_plan(m, N, KS, R, tile, G)
    print(name, "CUs", G, "R", R, plan)
    assert plan["fits"], (name, plan)
    if regime == "ge3x2":   # R from the CU count
        assert plan["nitems"] // G >= 3 and plan["D"] >= 2 * G, (name, plan)
    elif G == 256:   # the fixed grids are sized for the MI355X's 256 CUs
        if regime == "ge3":
            assert plan["nitems"] // G >= 3 and plan["D"] > 0, (name, plan)
        else:
            assert plan["nitems"] < 2 * G and plan["D"] == 0, (name, plan)
    A = kept.random_A(m)
    fixed = dict(maxiter=T, stop_rule=0)
    base, binfo = kept.base(("fixed", tile, m, R), lambda: run_engine(A, {"WTA_TILE": tile, **ARMS["sk0"]}, R, **fixed))
    assert_stream_k_ran(binfo, "sk0", name)
    assert binfo["panels_first"] == plan["panels"] and binfo["iterations_enqueued"] == T, (name, binfo, plan)
    assert binfo["wta_" + tile] == T, (name, binfo)
    assert np.array_equal(base.iters, np.full(NK * R, T, dtype=np.int32)) and not base.stopped_early.any()
    wraps = 1 if "WTA_SK_EPOCH0" in extra else 0   # the hook was read and the six launches crossed the wrap, once
    assert binfo["sk_wraps"] == 0, (name, binfo)
    for arm in ("sk1", "nowait"):
        r, info = run_engine(A, {"WTA_TILE": tile, **extra, **ARMS[arm]}, R, **fixed)
        assert_stream_k_ran(info, arm, name, launches=T)
        assert info["sk_wraps"] == wraps, (name, arm, info)
        assert info["panels_first"] == plan["panels"], (name, info, plan)
        assert_same_bits(r, base, (name, arm))
        del r
    j = 5   # one job against the oracle too
    W0, H0 = oracle.init_restart(SEED + j, m, N, KS[j % NK])
    Wo, Ho, _ = oracle.nmf_mu(A, W0, H0, T, 0)
    assert relfro(base.W[j], Wo) < TOL and relfro(base.H[j], Ho) < TOL, (relfro(base.W[j], Wo), relfro(base.H[j], Ho))


# ---- b. restarts that stop while stream-K is still launching ----

M_STOP, R_STOP = 4200, 160
STOP_CASES = {
    # never compacted, no narrow tail: every launch is the stream-K tile over the first packing
    "big-packed-once": {"WTA_TILE": "big", "REPACK_DIV": 1, "NARROW": 0},
    "mid-packed-once": {"WTA_TILE": "mid", "REPACK_DIV": 1, "NARROW": 0},
    # the real repack policy, tile choice and narrow tail
    "default-schedule": {},
}


@pytest.mark.parametrize("name", list(STOP_CASES))
def test_stopping_restarts_three_arms(kept, name):
    env = STOP_CASES[name]
    A = kept.planted_A(M_STOP)
    G = ncu()
    for tile in ("big", "mid"):
        if env.get("WTA_TILE", tile) == tile:
            plan = sk_plan(M_STOP, N, KS, R_STOP, tile, G)
            print(name, tile, "CUs", G, plan)
            assert plan["fits"], (name, tile, plan)
    rule = dict(maxiter=MAXITER, stop_rule=STOP_RULE)
    base, binfo = kept.base(("stop", name), lambda: run_engine(A, {**env, **ARMS["sk0"]}, R_STOP, **rule))
    assert_stream_k_ran(binfo, "sk0", name)
    print(name, "iterations", int(base.iters.min()), "..", int(base.iters.max()), "seconds", base.seconds_total)
    for arm in ("sk1", "nowait"):
        r, info = run_engine(A, {**env, **ARMS[arm]}, R_STOP, **rule)
        print(name, arm, "seconds", r.seconds_total)
        lo, hi = int(r.iters.min()), int(r.iters.max())
        # not vacuous: every job stopped by the rule, at widely spread iterations, and stream-K launched after the first
        # stop (so over groups that hold stopped restarts)
        assert np.array_equal(r.stopped_early, np.ones(NK * R_STOP, dtype=np.int32)) and hi < MAXITER, (name, arm, lo, hi)
        assert hi >= 2 * lo, (name, arm, lo, hi)
        if "REPACK_DIV" in env:
            assert_stream_k_ran(info, arm, name, launches=info["iterations_enqueued"])
            assert info["repacks"] == 0 and info["panels_min"] == info["panels_first"], (name, arm, info)
            assert info["iterations_enqueued"] >= hi, (name, arm, info)   # to natural completion: wholly dead groups
        else:
            assert_stream_k_ran(info, arm, name)
            assert info["repacks"] >= 1, (name, arm, info)
        assert info["wta_sk"] > lo, (name, arm, info, lo)
        assert_same_bits(r, base, (name, arm))
        del r


# ---- c. two restart groups at a stream-K grid ----

@pytest.mark.parametrize("rule", ["fixed40", "stop"])
def test_two_restart_groups_at_a_stream_k_grid(kept, rule):
    """Two engines on one GPU, each running the R = 160 grid of (a) / (b) in stream-K form from its own host thread,
    against one-engine NMFC_WTA_SK=0 runs of the same two job ranges.  Whether the groups' launches overlapped on the
    GPU, and whether any continuation's poll timed out, is not observed: the results of the configuration are pinned,
    not the event."""
    from nmfconsensus_amd.distributed import RestartGroups
    R = 2 * R_STOP
    A = kept.planted_A(M_STOP)
    kw = dict(maxiter=40, stop_rule=0) if rule == "fixed40" else dict(maxiter=MAXITER, stop_rule=STOP_RULE)
    kw = {"seed": SEED, "want_factors": True, "want_counts": False, **kw}
    half = NK * R_STOP
    assert sk_plan(M_STOP, N, KS, R_STOP, "big", ncu())["fits"]
    with knobs({"WTA_SK": 1}), RestartGroups(A, device=0, groups=2) as grp:
        r = grp.run(KS, R, **kw)
        infos = [eng.last_run_info() for eng in grp.engines]
    assert r.extras.get("groups") == 2 and len(r.iters) == 2 * half
    for g, info in enumerate(infos):
        if rule == "fixed40":
            assert_stream_k_ran(info, "sk1", (rule, "group", g), launches=40)
        else:
            assert_stream_k_ran(info, "sk1", (rule, "group", g))
            assert info["wta_sk"] > int(r.iters[g * half:(g + 1) * half].min()), (rule, g, info)
    if rule == "stop":
        assert r.stopped_early.all() and int(r.iters.max()) < MAXITER
    from nmfconsensus_amd.nmf import Engine
    with knobs({"WTA_SK": 0}), Engine(A) as eng:
        for g in range(2):
            one = eng.run(KS, R, job_begin=g * half, job_end=(g + 1) * half, **kw)
            assert_stream_k_ran(eng.last_run_info(), "sk0", (rule, "one engine", g))
            assert len(one.iters) == half
            assert_same_bits(r, one, (rule, "group", g), offset=g * half)
            del one
