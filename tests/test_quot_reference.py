"""The cases of tests/test_gpu_brunet_quot.py (tests/quot_cases.py), pinned before any GPU sees them.  No GPU.

  * every batch of every regime stays inside the contract of brunet.hip's recip_batch: operands in [2^-204, 2^100],
    every prefix product inside [2^-1021, 2^1021], numerators zero or in [2^-30, 2^64];
  * the hard cases are what they claim, in exact integers: A 2^54 = P Q' - s with Q' odd in [2^53, 2^54), the correctly
    rounded quotient is the neighbour of the midpoint Q' that the sign of s selects, and numpy's a / p returns it -- so
    numpy is the correctly rounded reference on the GPU side;
  * the threshold below which quot_r's residual a - p q0 leaves the doubles is 2^-969, from the bit positions;
  * the exact-integer judge (quot_cases.faithful) accepts both neighbours of an inexact quotient and nothing else."""
from fractions import Fraction

import numpy as np
import pytest

import quot_cases as qc

IDS = [qc.regime_id(r) for r in qc.REGIMES]


def test_regime_list():
    names = {(r[0], r[1]) for r in qc.REGIMES}
    assert {("mid", n) for n in range(1, 6)} | {("low", 5), ("high", 5)} <= names          # recip_check.cpp's seven
    assert {("alt-from-low", 5), ("alt-from-high", 5), ("ascending", 5), ("descending", 5)} <= names
    assert {(f"four-{x}@{i}", 5) for x in ("low-high", "high-low") for i in range(5)} <= names
    assert len(names) == len(qc.REGIMES)


@pytest.mark.parametrize("index", range(len(qc.REGIMES)), ids=IDS)
def test_regime_inside_the_contract(index):
    name, n, slots, arange, zeros = qc.REGIMES[index]
    a, p = qc.regime_pairs(index)
    assert a.size == p.size >= qc.PAIRS and a.size % n == 0 and a.size < qc.PAIRS + n
    assert np.all(p >= 2.0 ** -204) and np.all(p < 2.0 ** 101) and np.all(np.isfinite(p))
    lo, hi = qc.prefix_exponent_span(p, n)
    print(f"{name} N={n}: prefix products within [2^{lo}, 2^{hi})")
    assert -qc.PREFIX_LIMIT <= lo and hi <= qc.PREFIX_LIMIT
    pos = a[a > 0]
    assert np.all(a >= 0) and pos.min() >= 2.0 ** arange[0] and pos.max() <= min(2.0 ** (arange[1] + 1), 2.0 ** 64)
    assert (np.count_nonzero(a == 0) > a.size // 32) == zeros
    assert not np.signbit(a).any()
    if name == "ascending":
        assert np.all(np.diff(p.reshape(-1, n), axis=1) >= 0)
    if name == "descending":
        assert np.all(np.diff(p.reshape(-1, n), axis=1) <= 0)
    if isinstance(slots, list):   # every slot draws from its own end
        e = np.frexp(p.reshape(-1, n))[1] - 1
        for i, (e0, e1) in enumerate(slots):
            assert e[:, i].min() == e0 and e[:, i].max() == e1
    # the order-adversarial regimes reach both ends of the interval inside one batch
    if zeros:
        e = np.frexp(p.reshape(-1, n))[1] - 1
        assert (e.max(axis=1) - e.min(axis=1)).max() >= 296


def test_hard_cases_exact():
    h = qc.hard_pairs()
    assert len(h["P"]) == qc.HARD_PAIRS >= 10 ** 5
    with np.errstate(under="ignore"):
        qn = h["a"] / h["p"]
    man, ex = np.frexp(qn)
    qint = np.ldexp(man, 54).astype(np.int64).tolist()    # the quotient in [0.5, 1) 2^(x - y) as a multiple of 2^-54
    a_man, p_man = np.ldexp(h["a"], -h["x"]), np.ldexp(h["p"], -h["y"])
    gaps = []
    for i, (P, Q, A, s) in enumerate(zip(h["P"], h["Q"], h["A"], h["s"])):
        assert P % 2 == 1 and (1 << 52) <= P < (1 << 53) and s % 2 != 0 and abs(s) <= 15
        assert Q % 2 == 1 and (1 << 53) <= Q < (1 << 54)
        assert (A << 54) == P * Q - s and 0 < A < (1 << 53)
        assert a_man[i] == A and p_man[i] == P                       # the doubles hold A 2^x and P 2^y exactly
        # A / P = (Q - s / P) 2^-54: the doubles next to it are (Q - 1) 2^-54 and (Q + 1) 2^-54, and it is nearer to
        # the one on the side of -s
        near, far = (Q - 1, Q + 1) if s > 0 else (Q + 1, Q - 1)
        assert abs((A << 54) - P * near) < abs((A << 54) - P * far)
        assert abs((A << 54) - P * near) == P - abs(s)               # |s| / P of a half-ulp from the midpoint
        assert ex[i] == h["x"][i] - h["y"][i] and qint[i] == near, i  # numpy's a / p is the correctly rounded one
        gaps.append(abs(s) / P)
    print(f"hard cases: distance from the midpoint {min(gaps):.3g} .. {max(gaps):.3g} of a half-ulp "
          f"(2^{np.log2(min(gaps)) - 54:.1f} .. 2^{np.log2(max(gaps)) - 54:.1f} relative)")
    e = np.frexp(h["p"])[1] - 1
    for e0, e1 in qc.HARD_P_RANGES:
        assert np.count_nonzero((e >= e0) & (e <= e1)) > qc.HARD_PAIRS // 8
    assert e.min() == -204 and e.max() == 100


@pytest.mark.parametrize("n", range(1, 6))
def test_hard_batches(n):
    a, p, slot = qc.hard_batches(n)
    h = qc.hard_pairs()
    assert a.size == n * qc.HARD_PAIRS and np.array_equal(a[slot], h["a"]) and np.array_equal(p[slot], h["p"])
    assert np.array_equal(slot // n, np.arange(qc.HARD_PAIRS)) and set((slot % n).tolist()) == set(range(n))
    lo, hi = qc.prefix_exponent_span(p, n)
    assert -qc.PREFIX_LIMIT <= lo and hi <= qc.PREFIX_LIMIT and np.all(a > 0)


@pytest.mark.parametrize("n", range(1, 6))
def test_tiny_numerators_and_the_residual_threshold(n):
    a, p = qc.tiny_pairs(n)
    assert a.min() >= 2.0 ** -1074 and a.max() < 2.0 ** -960 and np.count_nonzero(a < 2.0 ** -1022) > a.size // 4
    assert p.min() >= 2.0 ** -60 and p.max() < 2.0 ** 101
    lo, hi = qc.prefix_exponent_span(p, n)
    assert -qc.PREFIX_LIMIT <= lo and hi <= qc.PREFIX_LIMIT
    above = a >= 2.0 ** qc.TINY_EXACT_EXP
    assert np.count_nonzero(above) > 1000 and np.count_nonzero(~above) > 1000
    # the last bit of the exact residual a - p q0 is the lower of a's and of p q0's, ulp(p) ulp(q0).  Any q0 within a
    # few ulp of a / p has the exponent of a / p or the one below; take the lower one.
    with np.errstate(under="ignore"):
        q0 = a / p
    last_bit = qc.ulp_exponent(p) + np.minimum(qc.ulp_exponent(q0), qc.ulp_exponent(np.nextafter(q0, 0.0)))
    last_bit = np.minimum(last_bit, qc.ulp_exponent(a))
    assert last_bit[above].min() >= -1074         # above the threshold every bit of the residual is a double's bit
    assert last_bit[~above].min() < -1074          # below it that is no longer so ...
    just_below = (~above) & (a >= 2.0 ** (qc.TINY_EXACT_EXP - 1))
    assert last_bit[just_below].min() == -1075     # ... starting right at the threshold


def test_threshold_is_tight_in_bit_positions():
    """e_a = -969 is the first exponent at which (e_a - 1) - 104, the lowest the last bit of p q0 can sit, is still a
    double's bit; the issue's example pair has an exact residual that rounds to zero."""
    assert (qc.TINY_EXACT_EXP - 1) - 104 == -1074 and (qc.TINY_EXACT_EXP - 2) - 104 < -1074
    a, p = 2.0 ** -1060, 1.5 * 2.0 ** -60
    q0 = a * (1.0 / p)
    res = Fraction(a) - Fraction(p) * Fraction(q0)
    assert res != 0 and abs(res) < Fraction(1, 2 ** 1075)


def test_faithful_judge():
    a = np.array([1.0, 1.0, 1.0, 1.0, 6.0, 6.0, 0.0, 2.0 ** -1070, 2.0 ** -1070])
    p = np.array([3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 7.0, 3.0, 3.0])
    third = 1.0 / 3.0                                   # rounded down: the exact quotient lies above it
    tiny = 2.0 ** -1070 / 3.0                           # 16 / 3 of 2^-1074 -> 5
    q = np.array([third, np.nextafter(third, 1.0), np.nextafter(third, 0.0), np.nextafter(np.nextafter(third, 1.0), 1.0),
                  2.0, np.nextafter(2.0, 3.0), 0.0, tiny, np.nextafter(tiny, 1.0)])
    assert tiny == 5 * 2.0 ** -1074
    assert qc.faithful(q, a, p).tolist() == [True, True, False, False, True, False, True, True, True]
