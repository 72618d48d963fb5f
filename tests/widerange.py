"""Wide-range inputs, extended-precision references and the componentwise bound of the element-by-element tests
(test_widerange_reference.py on the CPU, test_gpu_widerange.py on the GPU).  Holds no tests.

Why: the suite's bar for W and H is a relative Frobenius error below 1e-9 on dense, evenly scaled inputs.  A norm
cannot see rows or columns that lie many decades below the largest one, and on evenly scaled data the constant
DIV_BY_ZERO_AVOIDANCE = 1e-9 (nmf_mu.c:56) is added to denominators of O(10..1000), where dropping or doubling it
moves the result by a few 1e-9 at most.  The data here spans many decades per row and per column, has exact zeros
where mu_rule's zero cases decide, and has denominators on both sides of 1e-9.

The metric.  The MU update (nmf_mu.c:174-216) and the Brunet KL update (brunet.hip's header) contain no subtraction: on
non-negative data every operation is a sum of non-negative products, a product or a quotient.  So the COMPONENTWISE
relative error of a correct fp64 implementation, in any summation order, fused or not, has a bound that needs no tuning.
In units of u = 2^-53, to first order:

  * a dot product of L non-negative terms has relative error at most (L + 1) u in any order (each product one
    rounding, at most L - 1 additions on the path of any term, nothing cancels; a fused multiply-add only removes
    roundings);
  * with the factors carrying relative errors dW and dH (in u), the numerator W^T A carries dW + (m + 1); the Gram
    matrix W^T W carries 2 dW + (m + 1); the denominator (W^T W) H carries 2 dW + dH + (m + 1) + (k + 1);
  * adding a positive constant (1e-9 in MU; eps in KL) never raises a relative error, it costs one rounding;
  * the quotient times the old factor then carries
        dH' = (dW + m + 1) + (2 dW + dH + m + k + 2) + dH + [add, divide, multiply: 3]
            = 3 dW + 2 dH + (2 m + k + 6),
    and "+ 8" instead of "+ 6" covers the KL quotient, which is faithful (2 u) instead of correctly rounded (1 u), and
    the final rounding of the reference to fp64 precision;
  * the W update is the same with the new H, n for m and the roles swapped: dW' = 3 dH' + 2 dW + (2 n + k + 8).
  * KL: A / (W H) carries dW + dH + (k + 1) + 1, its product sum with W over the m genes dW more and (m + 1), the column
    sums of W dW + m: (H * G + eps) / colSums(W) carries 3 dW + 2 dH + 2 m + k + 6, inside the same recursion.

So, from dH = dW = 0, T times:
        dH <- 3 dW + 2 dH + (2 m + k + 8)
        dW <- 3 dH + 2 dW + (2 n + k + 8)
For (1000, 40, 5): 2 013 u for H and 6 132 u for W at T = 1 (about 7e-13), about 85 000 u at T = 2.  The fp64 oracle
sits one to three orders below the bound (test_widerange_reference.py prints its figures); the bound at T = 1 sits
more than a thousand times below 1e-9.
Exact zeros (mu_rule's old == 0 || num == 0) are compared exactly: a zero where the reference has none, or the reverse,
is an error of any size.

The data.  wide_A: A[i, j] = alpha r_i c_j U(0.05, 1), r_i = 10^U(-6, 6), c_j = 10^U(-6, 6), about 30 % exact zeros, row
5 % m and column 3 % n all zero, the smallest row scales on the structural edges (row m - 1 and the rows of the last
partial 16-, 64- and 128-row blocks, at most a quarter of the rows), the smallest column scale on column n - 1.
wide_init: W0[i, :] = s_i U(0.05, 1), s_i = 10^U(-12, 0), H0[:, j] = t_j U(0.05, 1), t_j = 10^U(-12, 0); for MU about 10 %
exact zeros in both and, for k >= 3, row 1 of H0 all zero; for KL no zeros and every entry inside brunet.hip's admitted
[2^-60, 2^60].  Job q of a batch (restart q of its k) has its own stream and its W0 times 2^(-8 (q % 5)): restarts
stacked side by side differ by up to 2^32 in scale, so a leak from a neighbour is far above the bound.

Where the recipe had to move to meet the conditions test_widerange_reference.py asserts (the bound never moved):
  * c_j spans 12 decades, not 6.  H <- H * (W^T A) / (...) ties the columns of H to c_j wherever the denominator is
    above 1e-9, and the KL update ties them exactly (the column sums of W H become those of A), so 6 decades leave
    1..3 % of the columns of H below 1e-9 of ||H||_F; the test wants a fifth.
  * the scales are drawn stratified (_log_uniform), so five or eight of them still cover the decades.
  * MU_W0_MK: above m k = 16384, W0 is scaled down to keep the H-side denominator on both sides of 1e-9.
  * KL_W0_SCALE: the KL factors times 2^20, to stay inside [2^-60, 2^60] under the batch scaling of 2^-32.
  * RESEED: ten MU (shape, k) cases take a later init seed, where the draw left one side's denominators one-sided.

The third kind, "euclid": the BROAD script's Euclidean NMF() in the Gram form the engine runs (ref_euclid),
H <- H * ((W^T A) / ((W^T W) H)) + eps, then W <- (W * (A H^T)) / (W (H H^T)) + eps with the new H, eps = 2^-52, no guard
and no clamp.  The same recursion bounds it: H is divide, multiply, add and W is multiply, divide, add, three roundings
each and inside the "+ 8"; nothing is subtracted, and adding the positive eps never raises a relative error.
The data is wide_A with a scale of its own (ALPHA["euclid"] = 1e-26) and wide_init with W0 times 2^-34
(EUCLID_W0_SCALE) and about 10 % exact zeros in W0 and in H0: the rule's products old * q then lie on both sides of eps
(test_widerange_reference.py asserts the shares), so an eps added twice, added before the divide or replaced by
another constant decides a third of the values.  A zero of W0 or H0, the all-zero row of A (a row of W) and the
all-zero column of A (a column of H) give exactly eps.  No row or column of W0 and no row or column of H0 is left
entirely zero (a zero mask that would make one gives up one entry).  The rule has no guard, so a denominator of 0 means
NaN: an all-zero row of W0 makes W (H H^T) zero in that row, an all-zero column of W0 makes a row of W^T W and with it
a row of (W^T W) H zero, and an all-zero column of H0 makes that column of (W^T W) H zero; the last is the one the
first recipe did not name.  An all-zero row of H0 harms no denominator (the row becomes eps); it is kept out with the
others so that every row of H0 takes part in the first update.  RESEED: 3001 x 150, k = 2 takes the init seed after
next, where only 15 of its 300 elements of H (exactly the 5 % asked for) had a product below eps / 8; now 22.

The KL corner cases (CORNER_*, below) are a second recipe: A and the caller factors at the ends of what
nmfc_brunet_create and nmfc_brunet_run admit.  The same reference and the same bound apply: there is no subtraction, so
the bound holds at any scale while everything stays normal, which test_widerange_reference.py asserts.
"""
import functools

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, \
    f"np.longdouble has eps {np.finfo(LD).eps}: the references of the wide-range tests need a 64-bit significand"

U = 2.0 ** -53
MU_EPS = 1e-9                       # DIV_BY_ZERO_AVOIDANCE, nmf_mu.c:56: the fp64 constant the kernels add
KL_EPS = 2.220446049250313e-16      # .Machine$double.eps, brunet.hip EPS

# global scale of A per update rule (conditions of test_widerange_reference.py: MU puts the W-side denominators on
# both sides of 1e-9; KL keeps A <= 2^64 and sum(A) <= 2^100)
ALPHA = {"mu": 10.0 ** -9.5, "kl": 1.0, "euclid": 1e-26}
EUCLID_EPS = 2.0 ** -52             # .Machine$double.eps, nmfc_common.hpp R_EPS: the constant the Euclidean rule adds
# Euclid: with A at 1e-26 and W0 at 2^-34 the products H0 * q and (W0 * num) / den of the first update lie on both
# sides of 2^-52 for every shape of EUCLID_BATCHES
EUCLID_W0_SCALE = 2.0 ** -34
# c_j = 10^U(-COL_DECADES, COL_DECADES): the columns of H scale with c_j (KL: with nothing else), and 6 decades in all
# cannot put a fifth of them 9 decades below the largest
COL_DECADES = 6.0
# MU: the H-side denominator (W^T W) H0 is about 0.003 m k t_j, so above m k = 16384 fewer than a tenth of the t_j would
# leave it below 1e-9; W0 is scaled down there (by 0.35 at 8192 x 16) to keep ||W0||^2 where it is at m k = 16384
MU_W0_MK = 16384.0
KL_W0_SCALE = 2.0 ** 20             # keeps s_i U(0.05, 1) 2^-32 >= 2^-60 (nmfc_brunet_run's check of caller factors)


def _rng(*key):
    return np.random.default_rng([int(x) for x in key])


def _log_uniform(rng, lo, hi, count):
    """count draws of 10^U(lo, hi), stratified: one per count-th of the range, in random order.  Each draw is still
    uniform in the exponent; the set covers the decades evenly at every count, so what the conditions of
    test_widerange_reference.py measure does not hang on the luck of five or eight draws."""
    return 10.0 ** (lo + (hi - lo) * (rng.permutation(count) + rng.random(count)) / count)


def edge_rows(m):
    """Row m - 1, then the rows of the last partial 16-, 64- and 128-row block, in that order of priority, at most
    m // 4 of them (m = 200 has 72 rows in its last partial 128-row block)."""
    out = [m - 1]
    for blk in (16, 64, 128):
        if m % blk:
            out += [i for i in range(m - 1, (m // blk) * blk - 1, -1) if i not in out]
    return out[:max(1, m // 4)]


def _place_smallest(scales, where):
    """The smallest scales onto the indices `where` (the very smallest first), the others keep their drawn order."""
    order = np.argsort(scales, kind="stable")
    small, rest = scales[order[:len(where)]], scales[np.sort(order[len(where):])]
    out = np.empty_like(scales)
    mask = np.ones(len(scales), dtype=bool)
    mask[where] = False
    out[where] = small
    out[mask] = rest
    return out


@functools.lru_cache(maxsize=None)
def wide_A(m, n, seed, kind="mu"):
    """The shared data matrix of a case (column-major fp64, read-only)."""
    rng = _rng(seed, m, n, 1)
    cdec = COL_DECADES
    r = _place_smallest(_log_uniform(rng, -6.0, 6.0, m), edge_rows(m))
    c = _place_smallest(_log_uniform(rng, -cdec, cdec, n), [n - 1])
    A = ALPHA[kind] * r[:, None] * c[None, :] * rng.uniform(0.05, 1.0, (m, n))
    A[rng.random((m, n)) < 0.30] = 0.0
    A[5 % m, :] = 0.0
    A[:, 3 % n] = 0.0
    A = np.asfortranarray(A)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def wide_init(m, n, k, seed, kind="mu", job=0):
    """(W0, H0) of job `job` of a case (column-major fp64, read-only)."""
    rng = _rng(seed, m, n, k, job, 2)
    s = _log_uniform(rng, -12.0, 0.0, m)
    t = _log_uniform(rng, -12.0, 0.0, n)
    W0 = s[:, None] * rng.uniform(0.05, 1.0, (m, k))
    H0 = rng.uniform(0.05, 1.0, (k, n)) * t[None, :]
    zw, zh = rng.random((m, k)) < 0.10, rng.random((k, n)) < 0.10
    if kind == "mu":
        W0 *= min(1.0, np.sqrt(MU_W0_MK / (m * k)))
        W0[zw] = 0.0
        H0[zh] = 0.0
        if k >= 3:
            H0[1, :] = 0.0
    elif kind == "euclid":
        # no row or column left entirely zero: the rule has no guard, and a zero denominator would make NaN
        for z in (zw, zh):
            for i in np.flatnonzero(z.all(axis=1)):
                z[i, i % z.shape[1]] = False
            for j in np.flatnonzero(z.all(axis=0)):
                z[j % z.shape[0], j] = False
        W0 *= EUCLID_W0_SCALE
        W0[zw] = 0.0
        H0[zh] = 0.0
    else:
        W0 *= KL_W0_SCALE
    W0 *= 2.0 ** (-8 * (job % 5))
    W0, H0 = np.asfortranarray(W0), np.asfortranarray(H0)
    W0.setflags(write=False)
    H0.setflags(write=False)
    return W0, H0


def wide_case(m, n, k, seed, kind="mu", job=0):
    """(A, W0, H0): the seeded wide-range case; A depends on (m, n, seed, kind) only, so the jobs of a batch share it."""
    return (wide_A(m, n, seed, kind),) + wide_init(m, n, k, seed, kind, job)


def ref_mu(A, W0, H0, T, eps=MU_EPS, want_den=False):
    """nmf_mu.c:174-216 in long double: H <- H * (W^T A) / ((W^T W) H + 1e-9), exactly 0 where H == 0 or W^T A == 0;
    then W <- W * (A H^T) / (W (H H^T) + 1e-9) with the new H and the same zero rule.  want_den: also the two
    denominators of the last iteration (before the constant)."""
    A, W, H = (np.asarray(x, dtype=LD) for x in (A, W0, H0))
    e = LD(eps)
    dh = dw = None
    for _ in range(T):
        num, dh = W.T @ A, (W.T @ W) @ H
        nz = (H != 0) & (num != 0)
        Hn = np.zeros_like(H)
        Hn[nz] = H[nz] * (num[nz] / (dh[nz] + e))
        H = Hn
        num, dw = A @ H.T, W @ (H @ H.T)
        nz = (W != 0) & (num != 0)
        Wn = np.zeros_like(W)
        Wn[nz] = W[nz] * (num[nz] / (dw[nz] + e))
        W = Wn
    return (W, H, dw, dh) if want_den else (W, H)


def ref_kl(A, W0, H0, T):
    """brunet.hip's header in long double: H <- (H * (W^T (A / (W H))) + eps) / colSums(W); then
    W <- (W * ((A / (W H)) H^T) + eps) / rowSums(H) with the new H."""
    A, W, H = (np.asarray(x, dtype=LD) for x in (A, W0, H0))
    e = LD(KL_EPS)
    for _ in range(T):
        H = (H * (W.T @ (A / (W @ H))) + e) / W.sum(axis=0)[:, None]
        W = (W * ((A / (W @ H)) @ H.T) + e) / H.sum(axis=1)[None, :]
    return W, H


def ref_euclid(A, W0, H0, T, trace=None):
    """The Euclidean NMF() update in the Gram form, in long double: H <- H * ((W^T A) / ((W^T W) H)) + eps, then
    W <- (W * (A H^T)) / (W (H H^T)) + eps with the new H; eps = 2^-52, no guard, no clamp.  trace: a list that receives,
    per iteration, a dict of every intermediate of both sides (numerator, Gram matrix, denominator, quotient, product;
    for H the product is the old * q the eps is added to, for W that is the quotient)."""
    A, W, H = (np.asarray(x, dtype=LD) for x in (A, W0, H0))
    e = LD(EUCLID_EPS)
    for _ in range(T):
        hnum, hgram = W.T @ A, W.T @ W
        hden = hgram @ H
        hq = hnum / hden
        hp = H * hq
        H = hp + e
        wnum, wgram = A @ H.T, H @ H.T
        wden = W @ wgram
        wp = W * wnum
        wq = wp / wden
        W = wq + e
        if trace is not None:
            trace.append(dict(Hnum=hnum, Hgram=hgram, Hden=hden, Hquot=hq, Hprod=hp,
                              Wnum=wnum, Wgram=wgram, Wden=wden, Wprod=wp, Wquot=wq))
    return W, H


REF = {"mu": ref_mu, "kl": ref_kl, "euclid": ref_euclid}


def bound_u(m, n, k, T):
    """(bound for H, bound for W) after T updates, in units of u = 2^-53: the recursion of the module docstring.  It
    holds for the MU, the KL and the Euclidean update alike: none of them subtracts, each elementwise rule is three
    roundings, and the constant each adds is positive."""
    dH = dW = 0
    for _ in range(T):
        dH = 3 * dW + 2 * dH + (2 * m + k + 8)
        dW = 3 * dH + 2 * dW + (2 * n + k + 8)
    return dH, dW


def cw_error(x, x_ref):
    """(number of elements whose zero state differs, worst |x - x_ref| / (u x_ref) over the others), every element
    counted: a non-finite x counts as an infinite error."""
    x = np.asarray(x, dtype=LD)
    x_ref = np.asarray(x_ref, dtype=LD)
    assert x.shape == x_ref.shape, (x.shape, x_ref.shape)
    assert np.all(np.isfinite(x_ref)) and np.all(x_ref >= 0)
    zr = x_ref == 0
    zero_diff = int(np.count_nonzero((x == 0) != zr))
    nz = ~zr
    if not nz.any():
        return zero_diff, 0.0
    err = np.abs(x[nz] - x_ref[nz]) / (LD(U) * x_ref[nz])
    err[~np.isfinite(err)] = np.inf
    return zero_diff, float(err.max())


def cw_check(x, x_ref, bound, what=""):
    """x == 0 exactly where x_ref == 0 and nowhere else; everywhere else |x - x_ref| <= bound u x_ref, for every
    element.  Returns the worst ratio |x - x_ref| / (u x_ref)."""
    zero_diff, worst = cw_error(x, x_ref)
    assert zero_diff == 0, f"{what}: {zero_diff} elements are zero on one side only"
    assert worst <= bound, f"{what}: worst componentwise error {worst:.4g} u exceeds the bound {bound} u"
    return worst


def below_norm(X, axis):
    """Fraction of the rows (axis = 1) or columns (axis = 0) of X whose norm is below 1e-9 of X's Frobenius norm:
    what the relative Frobenius bar of 1e-9 cannot see."""
    X = np.asarray(X, dtype=LD)
    part = np.sqrt((X * X).sum(axis=axis))
    return float(np.mean(part < LD(1e-9) * np.sqrt((X * X).sum())))


# ---- the cases of test_gpu_widerange.py; test_widerange_reference.py pins each (shape, k) on the CPU first ---------

SEED = 20261019
# Engine.run batches: (m, n, ks, R, environment)
MFMA_BATCHES = [(1100, 72, (2, 7, 10, 16), 3, {}), (3001, 150, (16, 9, 2), 2, {}),
                (130, 17, (2, 3), 2, {"NMFC_SMALL": "0"}), (97, 33, (5,), 2, {"NMFC_SMALL": "0"})]
SMALL_BATCHES = [(m, n, (2, 5, 6, 8, 9, 16), 2, {"NMFC_SOLO": "0"}) for m in (200, 300, 1000) for n in (16, 40, 64)]
SOLO_BATCHES = [(m, n, ks, 2, {}) for (m, n) in ((1000, 40), (700, 30)) for ks in ((2, 3, 4, 5, 8), (2, 3, 4, 5, 8, 9))]
SOLO_DIRECT = [(1000, 40, k) for k in range(2, 9)] + [(1024, 30, 4), (129, 21, 4), (129, 21, 6), (37, 5, 5), (9, 8, 8)]
TEAM = [(129, 17, 3), (1024, 64, 7), (2000, 38, 3), (8192, 64, 16), (8100, 33, 2)]
GENERIC = [(129, 33, 1), (300, 60, 20), (500, 50, 24)]
DROPIN = [("generic", 129, 33, 1), ("solo", 1000, 40, 3), ("team", 1024, 64, 7), ("batch1", 8300, 40, 3),
          ("batch1", 300, 70, 3)]
KL_SHAPES = [(64, 5, (2,)), (333, 77, (7,)), (257, 256, (16,)), (603, 300, (2, 5, 10, 16))]
# one case per MU path for the T = 40 run against the oracle (zero pattern, relfro < 1e-9)
# (cases whose smallest value stays above 1e-250 for 40 iterations: where the denominator is far below 1e-9 an entry
# shrinks by num / 1e-9 per iteration, and e.g. 37 x 5 would reach the subnormals)
T40_PATHS = [("mfma", 130, 17, 3), ("small", 300, 40, 5), ("solo_batch", 1000, 40, 4), ("solo", 1024, 30, 4),
             ("team", 1024, 64, 7), ("generic", 300, 60, 20)]
T40_CASES = sorted({c[1:] for c in T40_PATHS})
NORM_CASES = [(130, 17, 1), (130, 17, 3), (130, 17, 16), (130, 17, 20), (3001, 151, 16)]


def mu_shapes():
    """Every (m, n, k) the MU tests of test_gpu_widerange.py run, once each, in a fixed order."""
    out = []
    for m, n, ks, _, _ in MFMA_BATCHES + SMALL_BATCHES + SOLO_BATCHES:
        out += [(m, n, k) for k in ks]
    out += SOLO_DIRECT + TEAM + GENERIC + [c[1:] for c in DROPIN]
    return sorted(set(out))


def kl_shapes():
    return sorted({(m, n, k) for m, n, ks in KL_SHAPES for k in ks})


# ---- the Euclidean NMF() rule (test_gpu_widerange.py::test_euclid_sweep) ----------------------------------------------
# Engine.run(euclid=) batches (m, n, ks, R, environment), the smallest shapes that reach every RULE_EUCLID instantiation
# of k_ahtw4: the 16-column narrow form, and the 64- and the 128-gene tile, each with and without the K-half skip (taken
# when n_pad - n >= 8, n_pad = n rounded up to 32).  200 x 60: n_pad - n = 4 and a ragged last gene tile; 1100 x 72:
# n_pad - n = 24; 3001 x 150: ragged last gene and sample tile.
_NO_NARROW = {"NMFC_NARROW": "0"}
EUCLID_BATCHES = [(97, 33, (5,), 2, {}), (130, 17, (2, 3), 2, {}),
                  (200, 60, (4,), 2, dict(_NO_NARROW, NMFC_AHTW_TILE="64")),
                  (200, 60, (4,), 2, dict(_NO_NARROW, NMFC_AHTW_TILE="128")),
                  (1100, 72, (2, 7, 10, 16), 3, {}), (1100, 72, (2, 7, 10, 16), 3, _NO_NARROW),
                  (1100, 72, (2, 7, 10, 16), 3, {"NMFC_AHTW_TILE": "128"}), (3001, 150, (16, 9, 2), 2, {})]
# the A h^T form each batch is there for, by position (the GPU test asserts that the run took it, from last_run_info)
EUCLID_FORMS = ["narrow", "narrow", "64", "128", "64-kskip", "64-kskip", "128-kskip", "64-kskip"]
EUCLID_ALL_FORMS = {"narrow", "64", "64-kskip", "128", "128-kskip"}
assert len(EUCLID_FORMS) == len(EUCLID_BATCHES) and set(EUCLID_FORMS) == EUCLID_ALL_FORMS
# runs that must give the same bits, by position: the two tiles of 200 x 60; 1100 x 72 under its three environments
EUCLID_SAME_BITS = [(2, 3), (4, 5), (4, 6)]


def euclid_kskip(n):
    """Whether the A h^T kernels skip the padding half of the last K stage at this n (engine.hip plan_chunk)."""
    return (n + 31) // 32 * 32 - n >= 8


assert all(("kskip" in f) == euclid_kskip(c[1]) for f, c in zip(EUCLID_FORMS, EUCLID_BATCHES) if f != "narrow")


def euclid_shapes():
    return sorted({(m, n, k) for m, n, ks, _, _ in EUCLID_BATCHES for k in ks})


def case_seed(kind, m, n, k):
    """The init seed of job 0 of a case: SEED, moved on for the cases of RESEED (where the luck of which large s_i
    meets which large r_i left one side's denominators all above or all below 1e-9)."""
    return SEED + RESEED.get((kind, m, n, k), 0)


RESEED = {("mu", 37, 5, 5): 1, ("mu", 200, 16, 6): 1, ("mu", 200, 40, 5): 1, ("mu", 200, 64, 5): 1, ("mu", 300, 40, 5): 1,
          ("mu", 300, 64, 2): 1, ("mu", 300, 70, 3): 1, ("mu", 1000, 16, 8): 2, ("mu", 1000, 40, 3): 1,
          ("mu", 3001, 150, 2): 5, ("euclid", 3001, 150, 2): 2}


# ---- the KL kernels at the corners of the domain they admit (test_gpu_widerange.py::test_kl_corners) -----------------
# nmfc_brunet_create admits A up to 2^64 and nmfc_brunet_run caller factors in [2^-60, 2^60]: on the first update VP =
# sum_c W H reaches about 2^+-118, and a group of restarts whose factors sit at opposite ends multiplies VP values some
# 2^236 apart in one batched reciprocal (brunet.hip recip_batch).  Kinds "kl-top", "kl-tiny", "kl-mixed" name the matrix;
# restart i of a batch takes the factor scales CORNER_SIGNS[i % 4], so every restart group of 2..5 holds both ends.
# 129 x 37 and 64 x 5: partial 256-lane tiles, partial TL = 64 operand tiles on both sides, n below a wave's 8 samples.
CORNER_KINDS = ("kl-top", "kl-tiny", "kl-mixed")
CORNER_SIGNS = ((59, 59), (59, -59), (-59, 59), (-59, -59))      # exponents of (W0, H0)
CORNER_KS = (2, 3, 4, 5, 6, 7, 8, 9, 10, 16)                     # every rank has its own RG / SPL / SL / RCP row
CORNER_CASES = [(kind, m, n, ks) for kind in CORNER_KINDS for m, n, ks in ((129, 37, CORNER_KS), (64, 5, (2,)))]
CORNER_T = 40    # on kl-tiny W grows by about m / n = 2^1.8 per iteration (eps decides both updates): not much longer


@functools.lru_cache(maxsize=None)
def corner_A(m, n, kind):
    rng = _rng(SEED, m, n, CORNER_KINDS.index(kind), 3)
    if kind == "kl-top":
        A = np.minimum(2.0 ** 64 * rng.uniform(0.5, 1.0, (m, n)), 2.0 ** 64)
        A[rng.random((m, n)) < 0.30] = 0.0
        A[0, 0] = 2.0 ** 64                       # the bound itself
    elif kind == "kl-tiny":
        A = 2.0 ** -200 * rng.uniform(0.5, 1.0, (m, n))
    else:
        A = np.ldexp(rng.uniform(0.5, 1.0, (m, n)), rng.integers(-60 + 1, 64 + 1, (m, n)).astype(np.int32))
    A = np.asfortranarray(A)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def corner_init(m, n, k, kind, job):
    rng = _rng(SEED, m, n, k, CORNER_KINDS.index(kind), job, 4)
    ew, eh = CORNER_SIGNS[job % 4]
    W0 = np.asfortranarray(rng.uniform(0.5, 1.0, (m, k)) * 2.0 ** ew)
    H0 = np.asfortranarray(rng.uniform(0.5, 1.0, (k, n)) * 2.0 ** eh)
    W0.setflags(write=False)
    H0.setflags(write=False)
    return W0, H0


def ref_kl_range(A, W0, H0, T):
    """ref_kl that also returns the smallest and largest VP = (W H)[i, j] either update divides by, and the smallest
    and largest entry of any W or H, over the T iterations."""
    A, W, H = (np.asarray(x, dtype=LD) for x in (A, W0, H0))
    e = LD(KL_EPS)
    vp, wh = [np.inf, 0.0], [np.inf, 0.0]

    def see(box, X):
        box[0], box[1] = min(box[0], X.min()), max(box[1], X.max())
    for _ in range(T):
        P = W @ H
        see(vp, P)
        H = (H * (W.T @ (A / P)) + e) / W.sum(axis=0)[:, None]
        P = W @ H
        see(vp, P)
        W = (W * ((A / P) @ H.T) + e) / H.sum(axis=1)[None, :]
        see(wh, W), see(wh, H)
    return W, H, tuple(vp), tuple(wh)


def case(kind, m, n, k, job=0):
    """(A, W0, H0) of job `job` of the case (kind, m, n, k) as the tests run it.  For a batch, `job` is the restart's
    index among the restarts of its k: restart 0 of every k is the case whose conditions the CPU test asserts."""
    if kind in CORNER_KINDS:
        return (corner_A(m, n, kind),) + corner_init(m, n, k, kind, job)
    return (wide_A(m, n, SEED, kind),) + wide_init(m, n, k, case_seed(kind, m, n, k), kind, job)


@functools.lru_cache(maxsize=None)
def reference(kind, m, n, k, job=0):
    """{T: (W, H)} of the long-double reference after T = 1 and T = 2 updates of case(kind, m, n, k, job): computed
    once, read-only."""
    A, W, H = case(kind, m, n, k, job)
    out = {}
    for T in (1, 2):
        W, H = REF.get(kind, ref_kl)(A, W, H, 1)
        W.setflags(write=False)
        H.setflags(write=False)
        out[T] = (W, H)
    return out


def prefetch(kind, m, n, k, jobs):
    """reference() of several jobs at once on a few threads (numpy's long-double loops release the GIL)."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(lambda j: reference(kind, m, n, k, j), jobs))


def measure_euclid(A, W0, H0):
    """The Euclidean case from its reference alone, over T = 1 and 2: the smallest denominator of each side (den_min:
    the rule divides without a guard); the smallest non-zero and the largest magnitude of any intermediate (numerator,
    Gram entry, denominator, quotient, product); and, of the first update, the shares of all elements of H and of W
    whose product old * q, the value eps is added to, is non-zero and below eps / 8 (lo) or above 8 eps (hi)."""
    trace = []
    ref_euclid(A, W0, H0, 2, trace=trace)
    out = {"Hden_min": np.inf, "Wden_min": np.inf, "min": np.inf, "max": 0.0}
    for it in trace:
        for side in "HW":
            out[f"{side}den_min"] = min(out[f"{side}den_min"], float(it[f"{side}den"].min()))
        for X in it.values():
            assert np.all(np.isfinite(X)) and np.all(X >= 0)
            out["max"] = max(out["max"], float(X.max()))
            if (X > 0).any():
                out["min"] = min(out["min"], float(X[X > 0].min()))
    e = LD(EUCLID_EPS)
    for side, p in (("H", trace[0]["Hprod"]), ("W", trace[0]["Wquot"])):
        out[f"{side}lo"] = float(np.mean((p > 0) & (p < e / 8)))
        out[f"{side}hi"] = float(np.mean(p > 8 * e))
    return out


def measure(kind, m, n, k, seed=None):
    """What test_widerange_reference.py asserts about a case, from the reference alone: the smallest fraction over
    T = 1, 2 of rows of W / columns of H below 1e-9 of the norm; for MU the fractions of the non-zero denominators of the
    first update below 1e-9 and above 1e-3 on each side; the smallest and largest positive value.  Euclid: what
    measure_euclid returns."""
    A = wide_A(m, n, SEED, kind)
    W0, H0 = wide_init(m, n, k, case_seed(kind, m, n, k) if seed is None else seed, kind, 0)
    if kind == "euclid":
        return measure_euclid(A, W0, H0)
    out = {"belowW": 1.0, "belowH": 1.0, "min": np.inf, "max": 0.0}
    for T in (1, 2):
        if kind == "mu":
            W, H, dw, dh = ref_mu(A, W0, H0, T, want_den=True)
            if T == 1:
                for side, d, x in (("W", dw, W), ("H", dh, H)):
                    d = d[x != 0]
                    out[f"{side}den_lo"] = float(np.mean(d < LD(1e-9))) if d.size else 0.0
                    out[f"{side}den_hi"] = float(np.mean(d > LD(1e-3))) if d.size else 0.0
        else:
            W, H = ref_kl(A, W0, H0, T)
        out["belowW"] = min(out["belowW"], below_norm(W, 1))
        out["belowH"] = min(out["belowH"], below_norm(H, 0))
        pos = np.concatenate([W[W > 0].ravel(), H[H > 0].ravel()])
        out["min"], out["max"] = min(out["min"], float(pos.min())), max(out["max"], float(pos.max()))
    return out
