"""numpy restatement of the BROAD nmfconsensus script's Euclidean NMF() (DESIGN.md "Euclidean NMF()"), the reference of
test_euclid_reference.py and test_gpu_euclid.py.

    set.seed(seed); W <- runif(m*k); H <- runif(k*n); eps <- .Machine$double.eps
    for t in 1..maxniter:
        VP <- W %*% H;  H <- H * (crossprod(W, V) / crossprod(W, VP)) + eps
        VP <- W %*% H;  W <- W * (V %*% t(H)) / (VP %*% t(H)) + eps
        if t %% stopfreq == 0: membership check (first row of each column's maximum, 1-based; old.membership starts 0)

Two forms: `literal` forms the m x n product VP as the script does (in fp64 or long double); `gram` forms the
denominators as (W^T W) H and W (H H^T) like the engine (fp64).  The inits are R's set.seed + runif through
pyoracle.Oracle().brunet_init, which exists on every machine the tests run on.
"""
import functools

import numpy as np

EPS = 2.0 ** -52


def membership(H):
    """order(H[, j], decreasing = TRUE)[1] per column: the first row of the maximum, 1-based."""
    return np.argmax(np.asarray(H), axis=0).astype(np.int32) + 1


def _update(V, W, H, eps, form):
    if form == "gram":
        H = H * ((W.T @ V) / ((W.T @ W) @ H)) + eps
        W = (W * (V @ H.T)) / (W @ (H @ H.T)) + eps
    else:
        VP = W @ H
        H = H * ((W.T @ V) / (W.T @ VP)) + eps
        VP = W @ H
        W = (W * (V @ H.T)) / (VP @ H.T) + eps
    return W, H


def run(V, W0, H0, maxiter, stopconv=40, stopfreq=10, *, form="literal", dtype=np.float64, fixed=False, trace=None,
        keep=None):
    """(W, H, t, stopped_early).  fixed: no stop rule, exactly maxiter iterations.  trace: a list that receives
    (t, no.change.count after the check) for every membership check.  keep: a dict that receives {t: (W, H)} after
    each iteration t it already has as a key."""
    V = np.asarray(V, dtype=dtype)
    W = np.array(W0, dtype=dtype)
    H = np.array(H0, dtype=dtype)
    eps = dtype(EPS)
    old = np.zeros(V.shape[1], dtype=np.int32)
    count = 0
    t = 0
    for t in range(1, maxiter + 1):
        W, H = _update(V, W, H, eps, form)
        if keep is not None and t in keep:
            keep[t] = (W, H)
        if not fixed and t % stopfreq == 0:
            new = membership(H)
            count = count + 1 if np.array_equal(new, old) else 0
            if trace is not None:
                trace.append((t, count))
            if count == stopconv:
                return W, H, t, 1
            old = new
    return W, H, t, 0


def frob(V, W, H):
    """sqrt(sum((V - W H)^2)) in long double."""
    ld = np.longdouble
    d = np.asarray(V, dtype=ld) - np.asarray(W, dtype=ld) @ np.asarray(H, dtype=ld)
    return float(np.sqrt(np.sum(d * d)))


@functools.lru_cache(maxsize=None)
def _oracle():
    from pyoracle import Oracle
    return Oracle()


def r_init(seed, m, n, k):
    """set.seed(seed); W <- runif(m*k) (m x k); H <- runif(k*n) (k x n)."""
    return _oracle().brunet_init(seed, m, n, k)


@functools.lru_cache(maxsize=None)
def planted(m, n):
    from nmfconsensus_amd.synthetic import planted_matrix
    A = planted_matrix(m, n)
    A.setflags(write=False)
    return A


# ---- the stop-rule jobs: planted matrices, k = 2..5, six restarts, under three (stopconv, stopfreq) settings ----------
STOP_SHAPES = {(1100, 72): 7000, (1000, 40): 9000}    # (m, n) -> nmfconsensus rseed (restart i runs set.seed(rseed + i))
STOP_KS = [2, 3, 4, 5]
STOP_R = 6
STOP_SETTINGS = [(40, 10), (5, 3), (1, 1)]
STOP_MAXITER = 2000
# jobs ((m, n), (stopconv, stopfreq), k, restart i) left out of the GPU comparison because the literal and the Gram
# fp64 forms themselves disagree there (test_euclid_reference.py finds them; at most one is allowed)
STOP_EXCLUDED = set()


@functools.lru_cache(maxsize=None)
def stop_reference(shape, setting, form="gram"):
    """{(k, i): (t, stopped_early, labels)} of every job of `shape` under `setting`, in nmfconsensus order."""
    m, n = shape
    V = planted(m, n)
    out = {}
    for k in STOP_KS:
        for i in range(1, STOP_R + 1):
            W0, H0 = r_init(STOP_SHAPES[shape] + i, m, n, k)
            _, H, t, early = run(V, W0, H0, STOP_MAXITER, setting[0], setting[1], form=form)
            out[(k, i)] = (t, early, membership(H))
    return out
