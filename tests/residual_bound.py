"""The derived bound of the residual-norm tests (test_residuals_reference.py on the CPU, test_gpu_residuals.py on the
GPU).  Holds no tests.

For fp64 factors W (m x k) and H (k x n), in long double:
    d*    = A - W H
    norm* = ||d*||_F / sqrt(m n)
    E     = (k + 2) u (|A| + |W||H|),  u = 2^-53
An fp64 evaluation of d, in any summation order, fused or not, has |d - d*| <= E per element (k products, k - 1
additions and the subtraction); the sum of m n squares in any order, the root and the division cost (m n + 2) u more:
    |dnorm - norm*|  <=  ||E||_F / sqrt(m n)  +  (m n + 2) u norm*
The bound of tests/test_gpu_widerange.py::test_calculate_norm_elementwise, with E in the place of the measured |d - d*|.
"""
import numpy as np

import widerange as wr

LD = wr.LD


def norm_and_bound(A, W, H):
    """(norm*, bound), both long double."""
    A, W, H = (np.asarray(x, dtype=LD) for x in (A, W, H))
    m, n = A.shape
    k = W.shape[1]
    assert W.shape == (m, k) and H.shape == (k, n)
    ds = A - W @ H
    mn = LD(m) * LD(n)
    norm_s = np.sqrt((ds * ds).sum()) / np.sqrt(mn)
    E = LD((k + 2) * wr.U) * (np.abs(A) + np.abs(W) @ np.abs(H))
    bound = np.sqrt((E * E).sum()) / np.sqrt(mn) + (mn + 2) * LD(wr.U) * norm_s
    return norm_s, bound


def within(value, norm_s, bound):
    return bool(np.isfinite(value)) and abs(LD(value) - norm_s) <= bound


def check(value, A, W, H, what):
    """Asserts the bound for `value`; prints the figure first.  Returns |value - norm*| / bound."""
    norm_s, bound = norm_and_bound(A, W, H)
    err = abs(LD(value) - norm_s)
    print(f"RES|{what}|dnorm {float(value):.17g}|error {float(err / (wr.U * norm_s)) if norm_s > 0 else float(err):.2f} u"
          f" of {float(bound / (wr.U * norm_s)) if norm_s > 0 else float(bound):.1f}")
    assert within(value, norm_s, bound), f"{what}: |dnorm - norm*| = {float(err):.3g} exceeds the bound {float(bound):.3g}"
    return float(err / bound) if bound > 0 else 0.0
