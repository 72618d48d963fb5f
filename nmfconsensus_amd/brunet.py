"""Brunet KL-divergence MU consensus (BASELINE.json configs[4]) on the HIP engine.

Host mirror of the BROAD `nmfconsensus(...)` R script that the reference names (commented-out call at
test_nmf.r:29) but does not ship.  Names and argument meaning follow that script:

  NMF_div(V, k, maxniter, seed, stopconv, stopfreq)      NMF.div: one Brunet KL-divergence restart
  NMF(V, k, maxniter, seed, stopconv, stopfreq)          NMF: one Euclidean (Frobenius) MU restart
  nmfconsensus(input_ds, k_init, k_final, num_clusterings, maxniter, error_function="divergence",
               rseed=123456789, stopconv=40, stopfreq=10)  the k sweep + consensus + cophenetic
                                                          (error_function "divergence" or "euclidean")

Every compute step calls nmfconsensus_amd/libnmf.so (nmfc_brunet_*, HIP gfx950); there is no CPU
fallback.  Restart i (1-based) of every k runs set.seed(rseed + i) then W <- runif(m k), H <- runif(k n)
(R's Mersenne-Twister, bit-exact).  NMF.div's error.v trace (a per-iteration log-sum over A, not used
by the consensus) is not computed; its value for the factors a run returns is (want_divergence, want_best: one device
pass per k batch, and only each k's best restart's factors leave the GPU).  Parity vs the reference is unpinned (the script is not in the
reference); the oracle is oracle/brunet_oracle.c.

error_function="euclidean" runs the script's NMF() on the fp64-MFMA engine of nmf.Engine (nmfc_engine_set_euclid:
the same three matrix products per iteration as nmf_mu, the script's elementwise rule, membership stop rule and
set.seed(rseed + i) seeding); DESIGN.md "Euclidean NMF()" restates the algorithm.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import BrunetOpts, Result
from .nmf import SweepResult, computeConsensusAndSaveFiles

__all__ = ["BrunetEngine", "NMF_div", "NMF", "nmfconsensus"]

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)


def _f64(a) -> np.ndarray:
    return np.asfortranarray(np.asarray(a, dtype=np.float64))


class BrunetEngine:
    """A resident data matrix on one MI355X plus the batched Brunet restart engine (nmfc_brunet_*)."""

    def __init__(self, A=None, device: int = -1, *, a_device_ptr: int | None = None, shape=None):
        self.L = _lib.lib()
        if a_device_ptr is not None:
            m, n = shape
            h = self.L.nmfc_brunet_create(device, ctypes.c_void_p(a_device_ptr), m, n, 1)
        else:
            A = _f64(A)
            m, n = A.shape
            self._A = A
            h = self.L.nmfc_brunet_create(device, A.ctypes.data_as(ctypes.c_void_p), m, n, 0)
        if not h:
            raise RuntimeError(f"nmfc_brunet_create failed: {_lib.last_error()}")
        self.h = h
        self.m, self.n = m, n
        self.device = self.L.nmfc_brunet_device(h)   # HIP ordinal resolved at creation (device -1: the current one)

    def close(self):
        if getattr(self, "h", None):
            self.L.nmfc_brunet_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_timing(self, on: bool):
        self.L.nmfc_brunet_set_timing(self.h, 1 if on else 0)

    def kernel_time(self, kid: int):
        """(launches, accumulated event ms, algorithmic flop per launch) of kernel kid (_lib.BK_*)."""
        ms, fl = ctypes.c_double(0.0), ctypes.c_double(0.0)
        cnt = self.L.nmfc_brunet_kernel_time(self.h, kid, ctypes.byref(ms), ctypes.byref(fl))
        return cnt, ms.value, fl.value

    def set_divergence(self, on: bool):
        """Later runs also compute every job's KL divergence (nmfc_brunet_set_divergence)."""
        self.L.nmfc_brunet_set_divergence(self.h, 1 if on else 0)
        self._divergence = bool(on)

    def divergence(self, nk: int, B: int) -> np.ndarray:
        """(nk, B) divergences of the last run's shard, which must have had them enabled (nmfc_brunet_divergence)."""
        out = np.zeros((nk, B), dtype=np.float64)
        if self.L.nmfc_brunet_divergence(self.h, out.ctypes.data_as(_dp)) != nk * B:
            raise RuntimeError(f"nmfc_brunet_divergence failed: {_lib.last_error()}")
        return out

    def best(self, ks):
        """(best_restart, best_divergence, best_W, best_H) per k of the last run's shard (nmfc_brunet_best): the restart
        with the smallest divergence, the lowest on ties, and its factors -- the only ones copied off the device."""
        m, n, nk = self.m, self.n, len(ks)
        br = np.zeros(nk, dtype=np.int32)
        bd = np.zeros(nk, dtype=np.float64)
        wflat = np.zeros(m * sum(ks), dtype=np.float64)
        hflat = np.zeros(n * sum(ks), dtype=np.float64)
        if self.L.nmfc_brunet_best(self.h, br.ctypes.data_as(_ip), bd.ctypes.data_as(_dp), wflat.ctypes.data_as(_dp),
                                   hflat.ctypes.data_as(_dp)) != nk:
            raise RuntimeError(f"nmfc_brunet_best failed: {_lib.last_error()}")
        Ws, Hs = [], []
        wo = ho = 0
        for k in ks:
            Ws.append(wflat[wo:wo + m * k].reshape((m, k), order="F"))
            Hs.append(hflat[ho:ho + k * n].reshape((k, n), order="F"))
            wo += m * k
            ho += k * n
        return [int(x) for x in br], [float(x) for x in bd], Ws, Hs

    def quot_probe(self, a, p, batch: int):
        """(q, r): the quotients a / p and the refined reciprocals of p as the KL kernels form them when `batch` (1..5)
        consecutive pairs share one hardware reciprocal (nmfc_brunet_quot_probe; a test diagnostic)."""
        a = np.ascontiguousarray(a, dtype=np.float64).ravel()
        p = np.ascontiguousarray(p, dtype=np.float64).ravel()
        if a.size != p.size:
            raise ValueError("a and p must have the same size")
        q, r = np.empty_like(a), np.empty_like(a)
        if self.L.nmfc_brunet_quot_probe(self.h, a.ctypes.data_as(_dp), p.ctypes.data_as(_dp), a.size, int(batch),
                                         q.ctypes.data_as(_dp), r.ctypes.data_as(_dp)) != 0:
            raise RuntimeError(f"nmfc_brunet_quot_probe failed: {_lib.last_error()}")
        return q, r

    def run(self, ks, R: int, *, maxiter: int = 2000, seed: int = 123456789, stopconv: int = 40, stopfreq: int = 10,
            restart_begin: int = 0, restart_end: int = -1, W_init=None, H_init=None, want_factors: bool = False,
            want_counts: bool = True, counts_device_ptr: int | None = None, verbose: bool = False,
            lanes: int = 0, want_divergence: bool = False, want_best: bool = False) -> SweepResult:
        """Jobs in nmfconsensus order (for k in ks: for i in restart shard); per-job arrays follow it.

        want_divergence: SweepResult.divergence, (nk, restarts of the shard), every job's KL divergence (NMF.div's
        error.v figure) on its final factors, from one device pass per k batch; want_best (implies want_divergence):
        best_restart, best_divergence, best_W, best_H, per k the restart with the smallest divergence and its factors,
        the only ones that leave the device.  Both hold for this call only; set_divergence() is restored after it."""
        ks = [int(k) for k in ks]
        nk = len(ks)
        rb = max(0, restart_begin)
        re = R if restart_end < 0 else min(restart_end, R)
        B = re - rb
        if B <= 0:
            raise ValueError("empty restart range")
        jk = [k for k in ks for _ in range(B)]
        nj = len(jk)
        o = BrunetOpts()
        self.L.nmfc_brunet_default_opts(ctypes.byref(o))
        o.maxiter, o.stopconv, o.stopfreq, o.seed = maxiter, stopconv, stopfreq, seed & 0xFFFFFFFF
        o.restart_begin, o.restart_end, o.verbose, o.lanes = rb, re, 1 if verbose else 0, lanes
        m, n = self.m, self.n
        res = Result()
        iters = np.zeros(nj, dtype=np.int32)
        early = np.zeros(nj, dtype=np.int32)
        labels = np.zeros((nj, n), dtype=np.int32)
        res.iters = iters.ctypes.data_as(_ip)
        res.stopped_early = early.ctypes.data_as(_ip)
        res.labels = labels.ctypes.data_as(_ip)
        counts = consensus = None
        if counts_device_ptr is not None:
            res.counts = ctypes.cast(ctypes.c_void_p(counts_device_ptr), _ip)
            res.counts_on_device = 1
        elif want_counts:
            counts = np.zeros((nk, n, n), dtype=np.int32)
            consensus = np.zeros((nk, n, n), dtype=np.float64)
            res.counts = counts.ctypes.data_as(_ip)
            res.consensus = consensus.ctypes.data_as(_dp)
        wflat = hflat = None
        if want_factors:
            wflat = np.zeros(sum(m * k for k in jk), dtype=np.float64)
            hflat = np.zeros(sum(k * n for k in jk), dtype=np.float64)
            res.W = wflat.ctypes.data_as(_dp)
            res.H = hflat.ctypes.data_as(_dp)
        wi = hi = None
        if W_init is not None or H_init is not None:
            if W_init is None or H_init is None:
                raise ValueError("W_init and H_init must be given together")
            wi = np.concatenate([_f64(w).reshape(-1, order="F") for w in W_init])
            hi = np.concatenate([_f64(h).reshape(-1, order="F") for h in H_init])
            if wi.size != sum(m * k for k in jk) or hi.size != sum(k * n for k in jk):
                raise ValueError("W_init/H_init sizes do not match the job shard")
        ks_arr = np.array(ks, dtype=np.int32)
        prev = getattr(self, "_divergence", False)
        want_divergence = want_divergence or want_best or prev
        if want_divergence != prev:
            self.set_divergence(want_divergence)
        try:
            rc = self.L.nmfc_brunet_run(self.h, ks_arr.ctypes.data_as(_ip), nk, R, ctypes.byref(o),
                                        wi.ctypes.data_as(_dp) if wi is not None else None,
                                        hi.ctypes.data_as(_dp) if hi is not None else None, ctypes.byref(res))
        finally:
            if want_divergence != prev:
                self.set_divergence(prev)
        if rc != 0:
            raise RuntimeError(f"nmfc_brunet_run failed: {_lib.last_error()}")
        div = self.divergence(nk, B) if want_divergence else None
        best = self.best(ks) if want_best else (None, None, None, None)
        Ws = Hs = None
        if want_factors:
            Ws, Hs = [], []
            wo = ho = 0
            for k in jk:
                Ws.append(wflat[wo:wo + m * k].reshape((m, k), order="F"))
                Hs.append(hflat[ho:ho + k * n].reshape((k, n), order="F"))
                wo += m * k
                ho += k * n
        return SweepResult(ks=ks, R=R, n=n, counts=counts, consensus=consensus, labels=labels, iters=iters,
                           stopped_early=early, W=Ws, H=Hs, seconds_total=res.seconds_total,
                           seconds_iterate=res.seconds_iterate, restart_iterations=res.restart_iterations,
                           max_iter_run=res.max_iter_run, job_begin=rb, job_end=re, divergence=div,
                           best_restart=best[0], best_divergence=best[1], best_W=best[2], best_H=best[3])


def NMF_div(V, k: int, maxniter: int = 2000, seed: int = 123456, stopconv: int = 40, stopfreq: int = 10,
            device: int = -1, want_divergence: bool = False, want_best: bool = False) -> dict:
    """NMF.div: one Brunet KL-divergence restart from set.seed(seed).  Returns dict(W, H, t); with want_divergence
    (or want_best, which for one restart asks the same) also 'divergence', error.v of the returned factors."""
    with BrunetEngine(V, device) as eng:
        # restart i = 1 of a one-restart sweep runs set.seed(rseed + 1)
        r = eng.run([k], 1, maxiter=maxniter, seed=seed - 1, stopconv=stopconv, stopfreq=stopfreq,
                    want_factors=True, want_counts=False, want_divergence=want_divergence or want_best)
    out = {"W": r.W[0], "H": r.H[0], "t": int(r.iters[0])}
    if r.divergence is not None:
        out["divergence"] = float(r.divergence[0, 0])
    return out


def _euclid_sweep(A, ks, R: int, *, maxiter: int, seed: int, stopconv: int, stopfreq: int, device: int = -1,
                  want_factors: bool = False, want_counts: bool = True, want_error: bool = False,
                  want_best: bool = False) -> SweepResult:
    """The Euclidean NMF() sweep on the MU engine, its per-job arrays reordered from the engine's job order (k
    fastest: job = restart * nk + k index) into nmfconsensus order (for k in ks: for restart i)."""
    from .nmf import Engine, INIT_R_RUNIF, LABEL_ARGMAX, STOP_REF_COMPAT

    ks = [int(k) for k in ks]
    nk = len(ks)
    with Engine(A, device) as eng:
        m, n = eng.m, eng.n
        # any stop rule but STOP_FIXED means NMF()'s membership rule in this mode
        r = eng.run(ks, R, maxiter=maxiter, seed=seed, stop_rule=STOP_REF_COMPAT, label_rule=LABEL_ARGMAX,
                    init_stream=INIT_R_RUNIF, want_factors=want_factors, want_counts=want_counts,
                    want_residuals=want_error, want_best=want_best, euclid=dict(stopconv=stopconv, stopfreq=stopfreq))
    perm = np.array([i * nk + g for g in range(nk) for i in range(R)], dtype=np.int64)
    scale = 1.0 / np.sqrt(float(m) * float(n))   # error.v = ||V - W H||_F / (m n) = dnorm / sqrt(m n)
    out = SweepResult(ks=ks, R=R, n=n, counts=r.counts, consensus=r.consensus, labels=r.labels[perm],
                      iters=r.iters[perm], stopped_early=r.stopped_early[perm],
                      W=[r.W[j] for j in perm] if r.W is not None else None,
                      H=[r.H[j] for j in perm] if r.H is not None else None, seconds_total=r.seconds_total,
                      seconds_iterate=r.seconds_iterate, restart_iterations=r.restart_iterations,
                      max_iter_run=r.max_iter_run, job_begin=0, job_end=R)
    if r.dnorm is not None:
        out.error = (r.dnorm[perm] * scale).reshape(nk, R)
    if want_best:
        out.best_restart = [r.best[k]["job"] // nk for k in ks]
        out.best_error = [r.best[k]["dnorm"] * scale for k in ks]
        out.best_W = [r.best[k]["W"] for k in ks]
        out.best_H = [r.best[k]["H"] for k in ks]
    return out


def NMF(V, k: int, maxniter: int = 2000, seed: int = 123456, stopconv: int = 40, stopfreq: int = 10,
        device: int = -1, want_error: bool = False) -> dict:
    """NMF: one Euclidean MU restart of the BROAD script from set.seed(seed).  Returns dict(W, H, t); with want_error
    also 'error', error.v of the returned factors: sqrt(sum((V - W H)^2)) / (m n)."""
    # restart i = 1 of a one-restart sweep runs set.seed(rseed + 1)
    r = _euclid_sweep(_f64(V), [k], 1, maxiter=maxniter, seed=seed - 1, stopconv=stopconv, stopfreq=stopfreq,
                      device=device, want_factors=True, want_counts=False, want_error=want_error)
    out = {"W": r.W[0], "H": r.H[0], "t": int(r.iters[0])}
    if r.error is not None:
        out["error"] = float(r.error[0, 0])
    return out


def nmfconsensus(input_ds, k_init: int, k_final: int, num_clusterings: int, maxniter: int,
                 error_function: str = "divergence", rseed: int = 123456789, directory: str | None = None,
                 stopconv: int = 40, stopfreq: int = 10, doc_string: str = "", device: int = -1,
                 want_divergence: bool = False, want_best: bool = False, want_error: bool = False) -> dict:
    """The BROAD consensus sweep: for k in k_init..k_final, num_clusterings Brunet restarts, membership
    = argmax of each H column, connectivity summed and divided by num_clusterings, then the cophenetic
    correlation, ordering and cutree membership (computeConsensusAndSaveFiles).  input_ds is an m x n
    array or a .gct path.  want_divergence adds 'divergence', (nk, num_clusterings); want_best adds that and 'best',
    {k: dict(restart=<0-based>, divergence=, W=<m x k>, H=<k x n>)}: the best metagenes per k.

    error_function="euclidean": the restarts are the script's NMF() (Frobenius objective) instead of NMF.div, with the
    same outputs.  want_error adds 'error', (nk, num_clusterings): error.v of every restart's final factors,
    sqrt(sum((V - W H)^2)) / (m n); want_best adds that and 'best', {k: dict(restart=, error=, W=, H=)}, per k the
    restart with the smallest error (the lowest on ties).  want_divergence is refused there (and want_error with
    "divergence")."""
    if error_function not in ("divergence", "euclidean"):
        raise ValueError("error_function must be 'divergence' or 'euclidean'")
    euclid = error_function == "euclidean"
    if euclid and want_divergence:
        raise ValueError("want_divergence belongs to error_function='divergence'; use want_error")
    if not euclid and want_error:
        raise ValueError("want_error belongs to error_function='euclidean'; use want_divergence")
    if k_init < 2 or k_final < k_init:
        raise ValueError("need 2 <= k_init <= k_final")
    if isinstance(input_ds, str):
        from .gct import read_gct
        A = read_gct(input_ds)[0]
    else:
        A = input_ds
    ks = list(range(k_init, k_final + 1))
    if euclid:
        sw = _euclid_sweep(_f64(A), ks, num_clusterings, maxiter=maxniter, seed=rseed, stopconv=stopconv,
                           stopfreq=stopfreq, device=device, want_error=want_error or want_best, want_best=want_best)
    else:
        with BrunetEngine(A, device) as eng:
            sw = eng.run(ks, num_clusterings, maxiter=maxniter, seed=rseed, stopconv=stopconv, stopfreq=stopfreq,
                         want_divergence=want_divergence, want_best=want_best)
    result = {str(k): sw.consensus[i] for i, k in enumerate(ks)}
    out = computeConsensusAndSaveFiles(result, save_dir=directory, doc_string=doc_string)
    out["sweep"] = sw
    if euclid:
        if want_error or want_best:
            out["error"] = sw.error
        if want_best:
            out["best"] = {k: dict(restart=sw.best_restart[i], error=sw.best_error[i], W=sw.best_W[i], H=sw.best_H[i])
                           for i, k in enumerate(ks)}
        return out
    if want_divergence or want_best:
        out["divergence"] = sw.divergence
    if want_best:
        out["best"] = {k: dict(restart=sw.best_restart[i], divergence=sw.best_divergence[i], W=sw.best_W[i],
                               H=sw.best_H[i]) for i, k in enumerate(ks)}
    return out
