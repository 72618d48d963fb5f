"""Every MU and KL kernel path, element by element, on wide-range data (tests/widerange.py).

The other GPU tests hold W and H to a relative Frobenius error of 1e-9 on dense, evenly scaled inputs: a norm cannot see
rows or columns many decades below the largest, and on even scales DIV_BY_ZERO_AVOIDANCE never decides a value.  Here
every path gets caller-provided W0 and H0 spanning twelve decades with exact zeros, runs T = 1 and T = 2 updates (MU:
FIXED; KL: a stopconv nothing reaches), and EVERY element of W and H is compared with the long-double reference
(widerange.ref_mu / ref_kl) under the derived componentwise bound (widerange.bound_u, no tuned tolerance): zero exactly
where the reference is zero, |x - x*| <= bound u x* everywhere else.  tests/test_widerange_reference.py pins the inputs,
the references and the conditions on the data on the CPU.

Labels, counts and consensus of every engine run are checked against numpy on the engine's own H (first maximum under
ARGMAX, first minimum under R_ORDER, ties included: the all-zero sample column gets label 1).  One case per MU path also
runs T = 40 against the fp64 oracle: identical zero pattern, relfro < 1e-9.  calculateNorm, the one place with a
subtraction, is held to its elementwise backward bound.  The KL kernels also run at the corners of the domain they admit
(widerange.CORNER_*: A at 2^64 or 2^-200, caller factors at 2^+-59 alternating inside every restart group).
The Euclidean NMF() rule (Engine.run(euclid=): k_hupdate and the five k_ahtw4 forms of RULE_EUCLID) runs on a wide case of
its own whose products lie on both sides of its constant 2^-52, under the same bound; where a factor or a row or column
of A is zero the result is exactly 2^-52 (test_euclid_sweep).

Every test prints the worst error in u = 2^-53 beside its bound (lines starting "WR|").
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import widerange as wr
from conftest import relfro

pytestmark = pytest.mark.gpu

TOL = 1e-9
NOSTOP = 10 ** 6   # a stopconv no restart reaches
FIXED, ARGMAX, R_ORDER = 0, 0, 1
DP = ctypes.POINTER(ctypes.c_double)


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


class Worst:
    """The worst componentwise error of a test per T, printed beside the bound."""

    def __init__(self, path):
        self.path, self.w = path, {}

    def check(self, kind, m, n, k, job, T, W, H):
        Wr, Hr = wr.reference(kind, m, n, k, job)[T]
        bh, bw = wr.bound_u(m, n, k, T)
        what = f"{self.path} {m}x{n} k={k} job {job} T={T}"
        eh = wr.cw_check(H, Hr, bh, what + " H")
        ew = wr.cw_check(W, Wr, bw, what + " W")
        key = (m, n, k, T)
        old = self.w.get(key, (0.0, 0.0))
        self.w[key] = (max(old[0], eh), max(old[1], ew))

    def report(self):
        for (m, n, k, T), (eh, ew) in sorted(self.w.items()):
            bh, bw = wr.bound_u(m, n, k, T)
            print(f"WR|{self.path}|{m}x{n}|k={k}|T={T}|H {eh:.0f} u of {bh}|W {ew:.0f} u of {bw}")


def check_labels(r, jobs_of_k, R, n, pick, zero_col=None):
    """Labels = first `pick` (argmax / argmin) of the run's own H, counts = label-equality sums, consensus = counts / R.
    jobs_of_k[i]: the job indices of the i-th k."""
    for j, H in enumerate(r.H):
        assert np.array_equal(r.labels[j], pick(H, axis=0) + 1), j
        if zero_col is not None:
            assert np.all(H[:, zero_col] == 0.0) and r.labels[j][zero_col] == 1, j   # an all-tie column: the first row
    for i, jobs in enumerate(jobs_of_k):
        lab = r.labels[jobs]
        assert len(jobs) == R
        cnt = np.sum(lab[:, :, None] == lab[:, None, :], axis=0)
        assert np.array_equal(r.counts[i], cnt), i
        assert np.array_equal(r.consensus[i], cnt / R), i


# ---- Engine.run batches: the MFMA sweep, k_small_mu, the solo kernels -------------------------------------------------

def engine_batch(path, m, n, ks, R, env, small):
    """One batch through Engine.run under `env`, T = 1 and 2, both label rules.  Job j has k = ks[j % nk] and is
    restart j // nk of its k: widerange job j // nk."""
    from nmfconsensus_amd.nmf import Engine
    nk = len(ks)
    jobs = [(ks[j % nk], j // nk) for j in range(nk * R)]
    for k in ks:
        wr.prefetch("mu", m, n, k, range(R))
    W0 = [wr.case("mu", m, n, k, q)[1] for k, q in jobs]
    H0 = [wr.case("mu", m, n, k, q)[2] for k, q in jobs]
    worst = Worst(path)
    with environ(env), Engine(wr.wide_A(m, n, wr.SEED)) as eng:
        for T in (1, 2):
            runs = []
            for rule in (ARGMAX, R_ORDER):
                r = eng.run(list(ks), R, maxiter=T, stop_rule=FIXED, label_rule=rule, W_init=W0, H_init=H0,
                            want_factors=True)
                assert eng.last_run_info()["small"] == small
                assert np.all(r.iters == T) and not r.stopped_early.any()
                runs.append(r)
            a, b = runs
            for j, (k, q) in enumerate(jobs):
                assert np.array_equal(a.W[j], b.W[j]) and np.array_equal(a.H[j], b.H[j]), j
                worst.check("mu", m, n, k, q, T, a.W[j], a.H[j])
            of_k = [list(range(i, nk * R, nk)) for i in range(nk)]
            check_labels(a, of_k, R, n, np.argmax, zero_col=3 % n)
            check_labels(b, of_k, R, n, np.argmin, zero_col=3 % n)
    worst.report()


def batch_id(c):
    return f"{c[0]}x{c[1]}-k{'_'.join(str(k) for k in c[2])}"


@pytest.mark.parametrize("kchunk", [None, "512"], ids=["default", "kchunk512"])
@pytest.mark.parametrize("case", wr.MFMA_BATCHES, ids=batch_id)
def test_mfma_sweep(case, kchunk):
    """The MFMA sweep engine (m_pad > 1024 or n > 64, or NMFC_SMALL=0) under the default schedule and NMFC_KCHUNK=512,
    the one family tests/test_gpu_schedule.py does not pin bit-identical to the default."""
    m, n, ks, R, env = case
    env = dict(env, **({"NMFC_KCHUNK": kchunk} if kchunk else {}))
    engine_batch("mfma" + ("-kchunk512" if kchunk else ""), m, n, ks, R, env, small=0)


@pytest.mark.parametrize("case", wr.SMALL_BATCHES, ids=batch_id)
def test_small_kernel(case):
    """k_small_mu (NMFC_SOLO=0): eight waves (m = 200, 1000), four (m = 300), both n_pad forms, ranks 2..16."""
    m, n, ks, R, env = case
    engine_batch("k_small_mu", m, n, ks, R, env, small=1)


@pytest.mark.parametrize("case", wr.SOLO_BATCHES, ids=batch_id)
def test_solo_batches(case):
    """Default knobs: ks 2..8 run in the fused k_solo_batch launch; with k = 9 beside them the per-rank solo launches
    run next to a k_small_mu block."""
    m, n, ks, R, env = case
    engine_batch("solo-batch" + ("+k9" if 9 in ks else ""), m, n, ks, R, env, small=1)


# ---- the Euclidean NMF() rule: k_hupdate and the five k_ahtw4 forms of RULE_EUCLID ---------------------------------------

EPS = wr.EUCLID_EPS
_euclid_runs = {}


def euclid_form(info, n):
    """The A h^T forms a run launched, from last_run_info: "narrow", "64" / "128", "-kskip" where n_pad - n >= 8."""
    skip = "-kskip" if wr.euclid_kskip(n) else ""
    return ({"narrow"} if info["ahtw_narrow"] else set()) | ({"64" + skip} if info["ahtw_64"] else set()) | \
           ({"128" + skip} if info["ahtw_128"] else set())


def euclid_batch(index):
    """Batch `index` of widerange.EUCLID_BATCHES through Engine.run(euclid=) under its environment, T = 1 and 2, both
    label rules: {T: (ARGMAX run, R_ORDER run)} and the set of A h^T forms launched.  Run once, kept for the
    comparisons between batches."""
    if index in _euclid_runs:
        return _euclid_runs[index]
    from nmfconsensus_amd.nmf import Engine
    m, n, ks, R, env = wr.EUCLID_BATCHES[index]
    nk = len(ks)
    jobs = [(ks[j % nk], j // nk) for j in range(nk * R)]
    W0 = [wr.case("euclid", m, n, k, q)[1] for k, q in jobs]
    H0 = [wr.case("euclid", m, n, k, q)[2] for k, q in jobs]
    out, forms = {}, set()
    with environ(env), Engine(wr.wide_A(m, n, wr.SEED, "euclid")) as eng:
        for T in (1, 2):
            runs = []
            for rule in (ARGMAX, R_ORDER):
                r = eng.run(list(ks), R, maxiter=T, stop_rule=FIXED, label_rule=rule, W_init=W0, H_init=H0,
                            want_factors=True, euclid=dict(stopconv=40, stopfreq=10))
                info = eng.last_run_info()
                assert info["small"] == 0
                assert info["ahtw_narrow"] + info["ahtw_64"] + info["ahtw_128"] == T, info
                forms |= euclid_form(info, n)
                assert np.all(r.iters == T) and not r.stopped_early.any()
                runs.append(r)
            out[T] = tuple(runs)
    _euclid_runs[index] = (out, forms)
    return _euclid_runs[index]


def euclid_id(index):
    m, n, ks, _, env = wr.EUCLID_BATCHES[index]
    return batch_id((m, n, ks)) + "".join(f"-{k[5:].lower()}{v}" for k, v in sorted(env.items()))


@pytest.mark.parametrize("index", range(len(wr.EUCLID_BATCHES)), ids=euclid_id)
def test_euclid_sweep(index):
    """Engine.run(euclid=) on the wide Euclidean case: every element of W and H of every job within bound_u of the
    long-double Gram form; exactly eps where W0 or H0 is zero (T = 1) and on the all-zero row and column of A; labels
    from the run's own H; the same bits under both label rules and under the environments of EUCLID_SAME_BITS."""
    m, n, ks, R, env = wr.EUCLID_BATCHES[index]
    nk = len(ks)
    jobs = [(ks[j % nk], j // nk) for j in range(nk * R)]
    for k in ks:
        wr.prefetch("euclid", m, n, k, range(R))
    runs, forms = euclid_batch(index)
    assert wr.EUCLID_FORMS[index] in forms, (forms, "the batch no longer takes the form it is here for")
    worst = Worst("euclid-" + "+".join(sorted(forms)))
    of_k = [list(range(i, nk * R, nk)) for i in range(nk)]
    for T in (1, 2):
        a, b = runs[T]
        for j, (k, q) in enumerate(jobs):
            assert np.array_equal(a.W[j], b.W[j]) and np.array_equal(a.H[j], b.H[j]), j
            worst.check("euclid", m, n, k, q, T, a.W[j], a.H[j])
            _, W0, H0 = wr.case("euclid", m, n, k, q)
            assert np.all(a.W[j][5 % m, :] == EPS) and np.all(a.H[j][:, 3 % n] == EPS), (j, T)
            if T == 1:
                assert (W0 == 0).any() and (H0 == 0).any()
                assert np.all(a.W[j][W0 == 0] == EPS) and np.all(a.H[j][H0 == 0] == EPS), j
        # the all-zero column of A holds eps in every row: a tie, so the first row under both rules
        check_labels(a, of_k, R, n, np.argmax)
        check_labels(b, of_k, R, n, np.argmin)
        assert np.all(a.labels[:, 3 % n] == 1) and np.all(b.labels[:, 3 % n] == 1)
    worst.report()
    for x, y in wr.EUCLID_SAME_BITS:
        if index in (x, y):
            other, _ = euclid_batch(x + y - index)
            for T in (1, 2):
                for j in range(nk * R):
                    assert np.array_equal(runs[T][0].W[j], other[T][0].W[j]), (x, y, T, j)
                    assert np.array_equal(runs[T][0].H[j], other[T][0].H[j]), (x, y, T, j)


def test_euclid_sweep_reaches_every_form():
    """The union of the forms the batches of EUCLID_BATCHES launched: the narrow form and the 64- and the 128-gene tile,
    each with and without the K-half skip."""
    seen = set()
    for index in range(len(wr.EUCLID_BATCHES)):
        seen |= euclid_batch(index)[1]
    print(f"WR|euclid|forms launched: {sorted(seen)}")
    assert seen >= wr.EUCLID_ALL_FORMS, seen


# ---- the single-restart entries ---------------------------------------------------------------------------------------

def mu_solo(A, W0, H0, T):
    from nmfconsensus_amd import _lib
    L = _lib.lib()
    m, n = A.shape
    k = W0.shape[1]
    assert L.nmfc_mu_solo_fits(m, n, k) == 1
    W, H = np.zeros((m, k), order="F"), np.zeros((k, n), order="F")
    it, early = ctypes.c_int(0), ctypes.c_int(0)
    rc = L.nmfc_mu_solo(A.ctypes.data_as(DP), m, n, k, T, FIXED, W0.ctypes.data_as(DP), H0.ctypes.data_as(DP),
                        W.ctypes.data_as(DP), H.ctypes.data_as(DP), ctypes.byref(it), ctypes.byref(early))
    assert rc == 0, _lib.last_error()
    assert it.value == T and not early.value
    return W, H


def mu_generic(A, W0, H0, T):
    from nmfconsensus_amd import _lib
    L = _lib.lib()
    m, n = A.shape
    k = W0.shape[1]
    W, H = W0.copy(order="F"), H0.copy(order="F")
    it, early = ctypes.c_int(0), ctypes.c_int(0)
    rc = L.nmfc_mu_generic(A.ctypes.data_as(DP), m, n, k, T, FIXED, W.ctypes.data_as(DP), H.ctypes.data_as(DP),
                           ctypes.byref(it), ctypes.byref(early))
    assert rc == 0, _lib.last_error()
    assert it.value == T and not early.value
    return W, H


def mu_team(A, W0, H0, T):
    from nmfconsensus_amd.nmf import Engine
    with Engine(A) as eng:
        W, H, it, early = eng.mu1(W0, H0, maxiter=T, stop_rule=FIXED)
    assert it == T and not early
    return W, H


def shape_id(c):
    return "x".join(str(v) for v in c)


@pytest.mark.parametrize("m,n,k", wr.SOLO_DIRECT, ids=[shape_id(c) for c in wr.SOLO_DIRECT])
def test_solo_direct(m, n, k):
    A, W0, H0 = wr.case("mu", m, n, k)
    worst = Worst("nmfc_mu_solo")
    for T in (1, 2):
        worst.check("mu", m, n, k, 0, T, *mu_solo(A, W0, H0, T))
    worst.report()


@pytest.mark.parametrize("m,n,k", wr.TEAM, ids=[shape_id(c) for c in wr.TEAM])
def test_team_kernel(m, n, k):
    A, W0, H0 = wr.case("mu", m, n, k)
    worst = Worst("k_team_mu")
    for T in (1, 2):
        worst.check("mu", m, n, k, 0, T, *mu_team(A, W0, H0, T))
    worst.report()


@pytest.mark.parametrize("m,n,k", wr.GENERIC, ids=[shape_id(c) for c in wr.GENERIC])
def test_generic_path(m, n, k):
    A, W0, H0 = wr.case("mu", m, n, k)
    worst = Worst("generic")
    for T in (1, 2):
        worst.check("mu", m, n, k, 0, T, *mu_generic(A, W0, H0, T))
    worst.report()


@pytest.mark.parametrize("arm,m,n,k", wr.DROPIN, ids=[shape_id(c) for c in wr.DROPIN])
def test_drop_in_nmf_mu(arm, m, n, k):
    """nmf_mu once per dispatch arm with maxiter = 2: REF_COMPAT cannot fire before iteration 400, so the result is the
    FIXED result after two updates."""
    from nmfconsensus_amd import _lib, libnmf
    L = _lib.lib()
    solo = bool(L.nmfc_mu_solo_fits(m, n, k)) and k <= 4
    m_pad = (m + 127) // 128 * 128
    want = "generic" if (k < 2 or k > 16) else "solo" if solo else "team" if (m_pad <= 8192 and n <= 64) else "batch1"
    assert want == arm   # the shape still takes the arm it is here for (compat.hip nmf_mu)
    A, W0, H0 = wr.case("mu", m, n, k)
    L.nmfc_nmf_mu_release()
    try:
        out = libnmf.nmf_mu(A, W0, H0, 2)
    finally:
        L.nmfc_nmf_mu_release()
    assert out["ret"] == 0 and out["maxiter"] == 2
    worst = Worst("nmf_mu-" + arm)
    worst.check("mu", m, n, k, 0, 2, out["w0"], out["h0"])
    worst.report()


# ---- zeros over a longer run ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path,m,n,k", wr.T40_PATHS, ids=[shape_id(c) for c in wr.T40_PATHS])
def test_forty_iterations_zero_pattern(oracle, path, m, n, k):
    """T = 40 FIXED on one case per MU path against the fp64 oracle: the zero pattern identical (no value underflows in
    these 40 iterations, test_widerange_reference.py), and the norm-wise bar of 1e-9."""
    from nmfconsensus_amd.nmf import Engine
    A, W0, H0 = wr.case("mu", m, n, k)
    T = 40
    if path in ("mfma", "small", "solo_batch"):
        env = {"mfma": {"NMFC_SMALL": "0"}, "small": {"NMFC_SOLO": "0"}, "solo_batch": {}}[path]
        with environ(env), Engine(A) as eng:
            r = eng.run([k], 1, maxiter=T, stop_rule=FIXED, W_init=[W0], H_init=[H0], want_factors=True)
            assert eng.last_run_info()["small"] == (0 if path == "mfma" else 1) and r.iters[0] == T
        W, H = r.W[0], r.H[0]
    else:
        W, H = {"solo": mu_solo, "team": mu_team, "generic": mu_generic}[path](A, W0, H0, T)
    Wo, Ho, _ = oracle.nmf_mu(A, W0, H0, T, FIXED)
    ew, eh = relfro(W, Wo), relfro(H, Ho)
    print(f"WR|T40-{path}|{m}x{n}|k={k}|T=40|relfro H {eh:.2e}|relfro W {ew:.2e}")
    assert np.array_equal(W == 0, Wo == 0) and np.array_equal(H == 0, Ho == 0)
    assert np.isfinite(W).all() and np.isfinite(H).all()
    assert ew < TOL and eh < TOL


# ---- the KL kernels ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big_batch():
    """B = NMFC_BR_SMALL_B + 5 of the built library: the grouped kernels with a partly filled last group and batched
    reciprocals of up to five quotients (tests/test_gpu_brunet_groups.py)."""
    from nmfconsensus_amd import _lib
    f = _lib.lib().nmfc_build_tuning_brunet
    f.restype = ctypes.c_char_p
    got = dict(kv.split("=", 1) for kv in f().decode().split(";"))
    return int(got["NMFC_BR_SMALL_B"], 0) + 5


@pytest.mark.parametrize("m,n,ks", wr.KL_SHAPES, ids=[batch_id(c) for c in wr.KL_SHAPES])
def test_kl_kernels(big_batch, m, n, ks):
    """BrunetEngine.run with caller factors: one restart, and B restarts of every k on one lane and on four.  Restart i
    has W0 times 2^(-8 (i % 5)), so the VP values a group's batched reciprocals multiply differ by many decades."""
    from nmfconsensus_amd.brunet import BrunetEngine
    worst = Worst("brunet")
    for k in ks:
        wr.prefetch("kl", m, n, k, range(big_batch))
    with BrunetEngine(wr.wide_A(m, n, wr.SEED, "kl")) as eng:
        for B, lanes in ((1, 1), (big_batch, 1), (big_batch, 4)):
            jobs = [(k, i) for k in ks for i in range(B)]   # nmfconsensus order: k-major
            W0 = [wr.case("kl", m, n, k, i)[1] for k, i in jobs]
            H0 = [wr.case("kl", m, n, k, i)[2] for k, i in jobs]
            for T in (1, 2):
                r = eng.run(list(ks), B, maxiter=T, stopconv=NOSTOP, W_init=W0, H_init=H0, want_factors=True,
                            lanes=lanes)
                assert np.all(r.iters == T) and not r.stopped_early.any()
                for j, (k, i) in enumerate(jobs):
                    worst.check("kl", m, n, k, i, T, r.W[j], r.H[j])
                # the label is the first row of the column maximum
                check_labels(r, [list(range(q * B, (q + 1) * B)) for q in range(len(ks))], B, n, np.argmax)
    worst.report()


# ---- calculateNorm: the one place with a subtraction ------------------------------------------------------------------

@pytest.mark.parametrize("m,n,k", wr.NORM_CASES, ids=[shape_id(c) for c in wr.NORM_CASES])
def test_calculate_norm_elementwise(m, n, k):
    """d = a - w h on the wide A with the twice-updated wide factors: |d - d*| <= (k + 2) u (|a| + |w||h|) per element
    (k products and k - 1 additions, fused or not, and the subtraction), and |norm - norm*| <= ||d - d*||_F / sqrt(m n)
    + (m n + 2) u norm* (the sum of m n squares in any order, the root and the division)."""
    from nmfconsensus_amd import libnmf
    LD = wr.LD
    A = wr.wide_A(m, n, wr.SEED)
    Wr, Hr = wr.reference("mu", m, n, k)[2]
    W, H = np.asfortranarray(Wr.astype(np.float64)), np.asfortranarray(Hr.astype(np.float64))
    v, d = libnmf.calculateNorm(A, W, H)
    wh = W.astype(LD) @ H.astype(LD)
    ds = A.astype(LD) - wh
    err = np.abs(d.astype(LD) - ds)
    lim = LD((k + 2) * wr.U) * (A.astype(LD) + wh)
    ratio = float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1), np.where(err > 0, np.inf, 0.0))))
    norm_s = np.sqrt((ds * ds).sum()) / np.sqrt(LD(m * n))
    nerr = abs(LD(v) - norm_s)
    nlim = np.sqrt((err * err).sum()) / np.sqrt(LD(m * n)) + LD((m * n + 2) * wr.U) * norm_s
    print(f"WR|calculateNorm|{m}x{n}|k={k}|worst |d - d*| at {ratio:.3f} of (k + 2) u (|a| + |w||h|)|"
          f"|norm - norm*| {float(nerr / (wr.U * norm_s)):.1f} u of {float(nlim / (wr.U * norm_s)):.1f}")
    assert np.isfinite(d).all() and np.isfinite(v)
    assert ratio <= 1.0
    assert nerr <= nlim


# ---- the KL kernels at the corners of the domain they admit ------------------------------------------------------------

@pytest.mark.parametrize("kind,m,n,ks", wr.CORNER_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in wr.CORNER_CASES])
def test_kl_corners(oracle, big_batch, kind, m, n, ks):
    """A at 2^64, at 2^-200 or spread over 2^-60..2^64, caller factors at 2^+-59 in the four sign combinations,
    restart i taking combination i % 4: every restart group multiplies VP values about 2^236 apart in one batched
    reciprocal.  T = 1 and 2: every element within the derived bound of the long-double reference.  T = 40: finite and
    within 1e-9 of the oracle.  Labels and counts from the run's own H; job 0 alone equals job 0 in the big batch."""
    from nmfconsensus_amd.brunet import BrunetEngine
    worst = Worst(f"corner-{kind}")
    for k in ks:
        wr.prefetch(kind, m, n, k, range(big_batch))
    A = wr.case(kind, m, n, ks[0])[0]
    alone = {}
    with BrunetEngine(A) as eng:
        for B in (1, big_batch):
            jobs = [(k, i) for k in ks for i in range(B)]
            W0 = [wr.case(kind, m, n, k, i)[1] for k, i in jobs]
            H0 = [wr.case(kind, m, n, k, i)[2] for k, i in jobs]
            of_k = [list(range(q * B, (q + 1) * B)) for q in range(len(ks))]
            for T in (1, 2, wr.CORNER_T):
                r = eng.run(list(ks), B, maxiter=T, stopconv=NOSTOP, W_init=W0, H_init=H0, want_factors=True)
                assert np.all(r.iters == T) and not r.stopped_early.any()
                check_labels(r, of_k, B, n, np.argmax)
                far = 0.0
                for j, (k, i) in enumerate(jobs):
                    if T <= 2:
                        worst.check(kind, m, n, k, i, T, r.W[j], r.H[j])
                    else:
                        assert np.isfinite(r.W[j]).all() and np.isfinite(r.H[j]).all(), (k, i)
                        Wo, Ho, _ = oracle.brunet(A, W0[j], H0[j], T, NOSTOP)
                        ew, eh = relfro(r.W[j], Wo), relfro(r.H[j], Ho)
                        far = max(far, ew, eh)
                        assert ew < TOL and eh < TOL, (k, i, ew, eh)
                    if i == 0 and B == 1:
                        alone[(k, T)] = (r.W[j], r.H[j])
                    elif i == 0:
                        assert np.array_equal(alone[(k, T)][0], r.W[j]) and np.array_equal(alone[(k, T)][1], r.H[j]), (k, T)
                if T > 2:
                    print(f"WR|corner-{kind}|{m}x{n}|B={B}|T={T}|worst relfro against the oracle {far:.2e}")
    worst.report()
