"""Operand pairs for the device probe of the KL kernels' quotient (nmfc_brunet_quot_probe: brunet.hip recip_batch and
quot_r), and the exact-integer helpers that judge its results.  Holds no tests: tests/test_quot_reference.py pins the
cases on the CPU, tests/test_gpu_brunet_quot.py runs them on the device.  Plain numpy and Python ints, fixed seeds.

A regime is a list of exponent ranges, one per slot of a batch of N quotients that share one v_rcp_f64: slot i of every
batch draws p = (random 52-bit mantissa) 2^e with e uniform in its range, so a regime fixes where in the admitted
interval [2^-204, 2^100] (brunet.hip, above recip_batch) each prefix product of the batch lands.

  * recip_check.cpp's seven: N = 1..5 at 2^-60..2^10, N = 5 at 2^-204..2^-200 and at 2^96..2^100; a in 2^-30..2^10.
  * order-adversarial batches over the whole interval: the two ends alternating (starting at either), exponents
    ascending and descending, four values at one end and one at the other in every position.  There a reaches 2^64
    (nmfc_brunet_create's bound on A) and one slot in sixteen holds a = 0.
  * hard cases: quotients next to a rounding midpoint (hard_pairs), inside batches whose other slots are random.
  * tiny numerators: a in [2^-1074, 2^-960], subnormals included, where quot_r's residual leaves the doubles.
"""
import functools
from fractions import Fraction

import numpy as np

PAIRS = 1 << 18           # pairs per (regime, N), rounded up to whole batches
LO, HI = (-204, -200), (96, 100)     # the ends of the admitted interval, as recip_check.cpp draws them
MID = (-60, 10)
WHOLE = (-204, 100)
A_RANGE = (-30, 10)       # recip_check.cpp's numerators
A_WIDE = (-30, 64)        # up to nmfc_brunet_create's bound on A (the mantissa is capped so that a <= 2^64)
PREFIX_LIMIT = 1021       # every prefix product of a batch stays inside [2^-1021, 2^1021]
RECIP_BAR = 2.0 ** -44    # |1 - p r|: the bar tests/test_brunet_recip.py holds the emulation to

# quot_r's residual fma(-p, q0, a), q0 = fl(a r): p q0 is a multiple of ulp(p) ulp(q0) = 2^(e_p - 52) 2^(e_q - 52), and
# q0 is within a few ulp of a / p, so e_p + e_q is e_a or e_a - 1: the exact residual's last bit can sit as low as
# 2^(e_a - 105).  It is a double's bit only from 2^-1074 up, i.e. for e_a >= -969.  (A subnormal q0, ulp 2^-1074, needs
# p > 2^1022 a >= 2^53 there, so ulp(p) >= 2 and the product's last bit is still a double's.)  Below 2^-969 the residual
# is rounded on the subnormal grid, for subnormal a usually to zero, and quot_r returns about a r.
TINY_EXACT_EXP = -969
TINY_RANGE = (-1074, -961)
TINY_P = (-60, 100)
TINY_REL = 2.0 ** -43     # below the threshold: |q - a / p| <= max(2^-43 |a / p|, 2^-1074)


def _rng(*key):
    return np.random.default_rng([20261020] + [int(x) for x in key])


def _draw(rng, erange, count):
    """count doubles with a random 52-bit mantissa and an exponent uniform in erange (both ends included)."""
    man = 1.0 + rng.integers(0, 1 << 52, count).astype(np.float64) / 2.0 ** 52
    return np.ldexp(man, rng.integers(erange[0], erange[1] + 1, count).astype(np.int32))


def _four_one(one_at, four, one):
    return [one if i == one_at else four for i in range(5)]


def regimes():
    """[(name, N, slots, a_range, zeros)]: slots is one exponent range per slot, or "asc" / "desc" (WHOLE, sorted)."""
    out = [(f"mid", n, [MID] * n, A_RANGE, False) for n in range(1, 6)]
    out += [("low", 5, [LO] * 5, A_RANGE, False), ("high", 5, [HI] * 5, A_RANGE, False)]
    for n in range(2, 6):
        out.append(("alt-from-low", n, [LO if i % 2 == 0 else HI for i in range(n)], A_WIDE, True))
        out.append(("alt-from-high", n, [HI if i % 2 == 0 else LO for i in range(n)], A_WIDE, True))
    out += [("ascending", 5, "asc", A_WIDE, True), ("descending", 5, "desc", A_WIDE, True)]
    for pos in range(5):
        out.append((f"four-low-high@{pos}", 5, _four_one(pos, LO, HI), A_WIDE, True))
        out.append((f"four-high-low@{pos}", 5, _four_one(pos, HI, LO), A_WIDE, True))
    return out


REGIMES = regimes()


def regime_id(reg):
    return f"{reg[0]}-N{reg[1]}"


@functools.lru_cache(maxsize=None)
def regime_pairs(index):
    """(a, p) of REGIMES[index], each of nb * N doubles, batch-major; read-only."""
    name, n, slots, arange, zeros = REGIMES[index]
    rng = _rng(1, index)
    nb = -(-PAIRS // n)
    if isinstance(slots, str):
        p = np.sort(_draw(rng, WHOLE, nb * n).reshape(nb, n), axis=1)
        if slots == "desc":
            p = p[:, ::-1]
    else:
        p = np.stack([_draw(rng, s, nb) for s in slots], axis=1)
    a = np.minimum(_draw(rng, arange, nb * n), 2.0 ** 64)
    if zeros:
        a[rng.random(nb * n) < 1.0 / 16] = 0.0
    a, p = np.ascontiguousarray(a), np.ascontiguousarray(p).reshape(-1)
    a.setflags(write=False)
    p.setflags(write=False)
    return a, p


def prefix_exponent_span(p, n):
    """(min, max) over every batch and every prefix c_i = p_0 ... p_i of the exact binary exponent of c_i's bounds:
    the smallest floor(log2) sum and the largest sum + i + 1 (each mantissa is below 2)."""
    e = np.frexp(np.asarray(p).reshape(-1, n))[1].astype(np.int64) - 1   # p = man 2^e, man in [1, 2)
    lo = np.cumsum(e, axis=1)
    hi = lo + np.arange(1, n + 1)[None, :]
    return int(lo.min()), int(hi.max())


# ---- hard cases --------------------------------------------------------------------------------------------------------

HARD_PAIRS = 1 << 17      # >= 10^5
HARD_S = (1, -1, 3, -3, 5, -5, 7, -7, 9, -9, 11, -11, 13, -13, 15, -15)
HARD_P_RANGES = (MID, LO, HI)


@functools.lru_cache(maxsize=None)
def hard_pairs():
    """HARD_PAIRS quotients next to a rounding midpoint.  P odd in [2^52, 2^53), s small and odd, Q' = s P^-1 mod 2^54
    kept when in [2^53, 2^54), A = (P Q' - s) / 2^54: then A / P = (Q' - s / P) / 2^54 with Q' odd, i.e. |s| / P of a
    half-ulp from the midpoint Q' 2^-54 of the doubles (Q' - 1) 2^-54 and (Q' + 1) 2^-54 -- about 2^-106 relative.
    Returns dict(P, Q, A, s: Python-int lists; a, p: doubles A 2^x, P 2^y scaled into the regimes; x, y: int arrays)."""
    rng = _rng(2)
    P, Q, A, S = [], [], [], []
    M = 1 << 54
    while len(P) < HARD_PAIRS:
        cand = (rng.integers(1 << 51, 1 << 52, 4096) * 2 + 1).tolist()   # odd, in [2^52, 2^53)
        ss = rng.integers(0, len(HARD_S), 4096).tolist()
        for pp, si in zip(cand, ss):
            s = HARD_S[si]
            q = (s * pow(pp, -1, M)) % M
            if q >= (1 << 53) and len(P) < HARD_PAIRS:
                P.append(pp), Q.append(q), A.append((pp * q - s) >> 54), S.append(s)
    n = HARD_PAIRS
    which = rng.integers(0, len(HARD_P_RANGES), n)
    lo = np.array([r[0] for r in HARD_P_RANGES])[which]
    hi = np.array([r[1] for r in HARD_P_RANGES])[which]
    y = (rng.integers(0, 1 << 30, n) % (hi - lo + 1) + lo - 52).astype(np.int32)           # p's exponent in its range
    x = (rng.integers(A_RANGE[0], A_RANGE[1] + 1, n) - 52).astype(np.int32)                # a in 2^-31 .. 2^11
    a = np.ldexp(np.array(A, dtype=np.float64), x)
    p = np.ldexp(np.array(P, dtype=np.float64), y)
    for v in (a, p, x, y):
        v.setflags(write=False)
    return dict(P=P, Q=Q, A=A, s=S, a=a, p=p, x=x, y=y)


@functools.lru_cache(maxsize=None)
def hard_batches(n):
    """(a, p, slot): HARD_PAIRS batches of n; batch j holds hard pair j in slot j % n, random mid-range pairs in the
    others.  slot: the flat index of each hard pair."""
    h = hard_pairs()
    rng = _rng(3, n)
    p = _draw(rng, MID, HARD_PAIRS * n)
    a = _draw(rng, A_RANGE, HARD_PAIRS * n)
    slot = np.arange(HARD_PAIRS) * n + np.arange(HARD_PAIRS) % n
    a[slot], p[slot] = h["a"], h["p"]
    for v in (a, p, slot):
        v.setflags(write=False)
    return a, p, slot


# ---- tiny numerators ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tiny_pairs(n):
    """(a, p) of -(-PAIRS // n) batches of n: a in [2^-1074, 2^-960] (np.ldexp rounds the mantissa onto the subnormal
    grid, never to zero), p in 2^-60 .. 2^100."""
    rng = _rng(4, n)
    count = -(-PAIRS // n) * n
    a = _draw(rng, TINY_RANGE, count)
    p = _draw(rng, TINY_P, count)
    assert np.all(a > 0)
    a.setflags(write=False)
    p.setflags(write=False)
    return a, p


def ulp_exponent(x):
    """e with ulp(x) = 2^e for positive doubles (subnormals: -1074)."""
    return np.maximum(np.frexp(x)[1].astype(np.int64) - 1, -1022) - 52


# ---- judging a quotient with exact integers ----------------------------------------------------------------------------

def faithful(q, a, p):
    """Boolean array: q[i] is the double just below or just above the exact a[i] / p[i] (or the quotient itself when it
    is a double).  numpy's a / p is the correctly rounded one; where q differs from it, q must be its neighbour on the
    side of the exact quotient, which is decided with exact rationals."""
    with np.errstate(under="ignore"):
        qn = a / p
    ok = q == qn
    for i in np.flatnonzero(~ok):
        qi, ni = float(q[i]), float(qn[i])
        if not np.isfinite(qi) or qi != float(np.nextafter(ni, qi)):
            continue
        exact = Fraction(float(a[i])) / Fraction(float(p[i]))
        ok[i] = min(qi, ni) < exact < max(qi, ni)
    return ok
