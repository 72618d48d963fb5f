"""The reference and the derived bound of the Brunet KL-divergence tests (test_kl_divergence_reference.py on the CPU,
test_gpu_brunet_divergence.py on the GPU).  Holds no tests.

For fp64 factors W (m x k) and H (k x n) and eps = 2^-52 (.Machine$double.eps), in long double:
    p*  = W H,   r* = (a + eps) / (p* + eps),   t* = a log r* - a + p*   (exactly p* where a = 0)
    D*  = sum t* / (m n)
This is NMF.div's error.v expression (oracle/brunet_oracle.c), which the device evaluates in fp64 as
    p = fma chain over q;  r = (a (+) eps) (/) (p (+) eps);  t = ((a (x) log r) (-) a) (+) p
with one rounding (u = 2^-53) per operation and a log good to L ulps.  To first order in u, per element:
    p            k roundings on sums of non-negative terms (fused or not, in any order):   |p - p*| <= k u p*
    a + eps      1 rounding;  p + eps: the error of p (k u p* <= k u (p* + eps)) and 1 rounding;  the quotient 1 more:
                 r = r* (1 + d),  |d| <= (k + 3) u
    log r        log r* + d, and the device log's own L ulps:   |lg - log r*| <= (k + 3) u + L u |log r*|
    a lg         1 rounding:   error <= (k + 3) u a + (L + 1) u a |log r*|
    (.) - a      1 rounding of a value of size at most a |log r*| + a:   + u (a |log r*| + a)
    (.) + p      the error of p and 1 rounding of t, |t*| <= a |log r*| + a + p*:   + k u p* + u (a |log r*| + a + p*)
    total        u [ (k + 5) a + (k + 1) p* + (L + 3) a |log r*| ]
which the bound below covers with a unit to spare on a and two on p (a fused a lg - a only drops a rounding):
    E = u [ (k + 6) a + (k + 3) p* + (L + 3) a |log r*| ]
The expression cancels (t* is small where p* is close to a while a and a |log r*| are not), so the bound is absolute
per element, not relative to t*.  The m n terms are added in some order (at most m n - 1 roundings of partial sums that
never exceed sum |t*| by more than first order) and divided by m n (2 more roundings with the product):
    |D - D*|  <=  ( sum E + (m n + 2) u sum |t*| ) / (m n)
L = 2: the error bound of the device log assumed here; the GPU test prints the worst error it observes on the fixtures'
own ratios (DESIGN.md 6c holds the figure).
"""
import numpy as np

import widerange as wr

LD = wr.LD
U = wr.U
EPS = 2.0 ** -52
L_LOG = 2


def terms(A, W, H):
    """(t*, a, p*, |log r*|) element by element, long double."""
    A, W, H = (np.asarray(x, dtype=LD) for x in (A, W, H))
    m, n = A.shape
    k = W.shape[1]
    assert W.shape == (m, k) and H.shape == (k, n)
    p = W @ H
    lg = np.log((A + LD(EPS)) / (p + LD(EPS)))
    t = np.where(A == 0, p, A * lg - A + p)
    return t, A, p, np.abs(lg)


def ref_kl_div(A, W, H):
    """D*, long double."""
    t = terms(A, W, H)[0]
    return t.sum() / (LD(t.shape[0]) * LD(t.shape[1]))


def div_and_bound(A, W, H, L=L_LOG):
    """(D*, bound), both long double."""
    t, a, p, alg = terms(A, W, H)
    k = np.asarray(W).shape[1]
    mn = LD(t.shape[0]) * LD(t.shape[1])
    E = LD(U) * (LD(k + 6) * a + LD(k + 3) * p + LD(L + 3) * a * alg)
    bound = (E.sum() + (mn + 2) * LD(U) * np.abs(t).sum()) / mn
    return t.sum() / mn, bound


def within(value, d_s, bound):
    return bool(np.isfinite(value)) and abs(LD(value) - d_s) <= bound


def check(value, A, W, H, what, ref=None):
    """Asserts the bound for `value`; prints the figure first.  `ref`: (D*, bound) when already known.  Returns
    |value - D*| / bound."""
    d_s, bound = ref if ref is not None else div_and_bound(A, W, H)
    err = abs(LD(value) - d_s)
    print(f"KLD|{what}|D {float(value):.17g}|error {float(err):.3e} of bound {float(bound):.3e}"
          f" ({float(err / bound) if bound > 0 else 0.0:.3f})")
    assert within(value, d_s, bound), f"{what}: |D - D*| = {float(err):.3g} exceeds the bound {float(bound):.3g}"
    return float(err / bound) if bound > 0 else 0.0


def log_ulp_error(x, y):
    """Worst |y - log x| in ulps of the fp64 result, y the fp64 logs under test of the fp64 values x, against logl."""
    x = np.asarray(x, dtype=np.float64)
    ref = np.log(x.astype(LD))
    ulp = np.spacing(np.abs(ref.astype(np.float64))).astype(LD)
    ok = ulp > 0
    return float(np.max(np.abs(np.asarray(y, dtype=np.float64).astype(LD) - ref)[ok] / ulp[ok])) if ok.any() else 0.0


def ratios(A, W, H):
    """The fp64 ratios (a + eps) / (p + eps) of a case, flattened: the arguments the device log sees (up to p's rounding)."""
    A, W, H = (np.asarray(x, dtype=np.float64) for x in (A, W, H))
    return ((A + EPS) / (W @ H + EPS)).ravel()
