"""The KL kernels' batched reciprocal and quotient (brunet.hip recip_batch / quot_r) on the device, to the ends of
their domain, through nmfc_brunet_quot_probe -- the kernels' own device functions, one batch per thread.

tests/test_brunet_recip.py checks a host restatement with an emulated v_rcp_f64; here the instruction itself runs:
  * every regime of tests/quot_cases.py (recip_check.cpp's seven and the order-adversarial batches over the whole
    admitted interval [2^-204, 2^100]): r finite, normal, |1 - p r| < 2^-44 in long double; q faithful, and equal to the
    correctly rounded a / p (the project's standing claim on random operands); a = 0 gives +0.0;
  * hard cases, quotients about 2^-106 from a rounding midpoint: faithful, and the number that are not the correctly
    rounded one is counted and printed, not bounded;
  * tiny numerators: faithful from 2^-969 up, within 2^-43 relative (or one subnormal step) below.
tests/test_quot_reference.py pins the cases and the threshold on the CPU.  Lines starting "QUOT|" are the figures
DESIGN.md section 15 quotes.

The kernels themselves at the corners they admit: tests/test_gpu_widerange.py::test_kl_corners."""
import numpy as np
import pytest

import quot_cases as qc

pytestmark = pytest.mark.gpu

LD = np.longdouble


@pytest.fixture(scope="module")
def eng():
    from nmfconsensus_amd.brunet import BrunetEngine
    e = BrunetEngine(np.ones((4, 4)))
    yield e
    e.close()


@pytest.fixture(scope="module")
def probed(eng):
    """probe(key, a, p, n) -> (q, r), each (key) run once on the device."""
    cache = {}

    def probe(key, a, p, n):
        if key not in cache:
            cache[key] = eng.quot_probe(a, p, n)
        return cache[key]
    return probe


def recip_error(p, r):
    """max |1 - p r| in long double (its own rounding, 2^-64, is 2^20 below the bar)."""
    return float(np.max(np.abs(LD(1) - p.astype(LD) * r.astype(LD))))


def check_recip(what, p, r):
    assert np.all(np.isfinite(r)) and np.all(np.abs(r) >= np.finfo(np.float64).tiny), what
    worst = recip_error(p, r)
    print(f"QUOT|recip|{what}|worst |1 - p r| = 2^{np.log2(worst):.2f}")
    assert worst < qc.RECIP_BAR, (what, np.log2(worst))


IDS = [qc.regime_id(r) for r in qc.REGIMES]


@pytest.mark.parametrize("index", range(len(qc.REGIMES)), ids=IDS)
def test_reciprocal(probed, index):
    name, n = qc.REGIMES[index][:2]
    a, p = qc.regime_pairs(index)
    q, r = probed(("regime", index), a, p, n)
    check_recip(f"{name}|N={n}", p, r)


@pytest.mark.parametrize("index", range(len(qc.REGIMES)), ids=IDS)
def test_quotient_random(probed, index):
    name, n = qc.REGIMES[index][:2]
    a, p = qc.regime_pairs(index)
    q, r = probed(("regime", index), a, p, n)
    zero = a == 0
    assert np.all(q[zero] == 0) and not np.signbit(q[zero]).any()       # exactly +0.0
    ok = qc.faithful(q, a, p)
    differ = int(np.count_nonzero(q != a / p))
    print(f"QUOT|random|{name}|N={n}|unfaithful {np.count_nonzero(~ok)}, not correctly rounded {differ} of {q.size}")
    assert ok.all(), (name, n, np.flatnonzero(~ok)[:5])
    assert differ == 0, (name, n, np.flatnonzero(q != a / p)[:5])


@pytest.mark.parametrize("n", range(1, 6))
def test_quotient_hard_cases(probed, n):
    a, p, slot = qc.hard_batches(n)
    q, r = probed(("hard", n), a, p, n)
    check_recip(f"hard|N={n}", p, r)
    assert qc.faithful(q, a, p).all()
    qh, ah, ph = q[slot], a[slot], p[slot]
    mis = int(np.count_nonzero(qh != ah / ph))
    print(f"QUOT|hard|N={n}|misrounded {mis} of {qh.size}")
    # the random slots of the same batches keep the standing claim
    rest = np.ones(q.size, dtype=bool)
    rest[slot] = False
    assert np.array_equal(q[rest], a[rest] / p[rest])


@pytest.mark.parametrize("n", range(1, 6))
def test_tiny_numerators(probed, n):
    a, p = qc.tiny_pairs(n)
    q, r = probed(("tiny", n), a, p, n)
    check_recip(f"tiny|N={n}", p, r)
    above = a >= 2.0 ** qc.TINY_EXACT_EXP
    ok = qc.faithful(q[above], a[above], p[above])
    assert ok.all(), (n, np.flatnonzero(~ok)[:5])
    al, pl, ql = a[~above].astype(LD), p[~above].astype(LD), q[~above].astype(LD)
    exact = al / pl                                                  # long double: 64 bits, no underflow down here
    err = np.abs(ql - exact)
    with np.errstate(under="ignore"):
        ulp = np.spacing(a[~above] / p[~above]).astype(LD)
    worst_ulp = float(np.max(err / ulp))
    off = err >= ulp                                                 # not faithful: a whole ulp or more away
    a_off = f"2^{np.log2(a[~above][off].max()):.1f}" if off.any() else "none"
    print(f"QUOT|tiny|N={n}|a >= 2^{qc.TINY_EXACT_EXP}: {np.count_nonzero(above)} faithful|below: worst error "
          f"{worst_ulp:.2f} ulp, {np.count_nonzero(off)} of {ql.size} an ulp or more off, the largest such a {a_off}")
    assert np.all(np.isfinite(q)) and np.all(q >= 0)
    assert np.all(err <= np.maximum(LD(qc.TINY_REL) * exact, LD(2.0) ** -1074))


def test_probe_arguments(eng):
    a = np.ones(6)
    for batch in (0, 6, 4):      # 4 does not divide 6
        with pytest.raises(RuntimeError, match="quot_probe"):
            eng.quot_probe(a, a, batch)
    q, r = eng.quot_probe(a * 3.0, a * 2.0, 3)
    assert np.array_equal(q, np.full(6, 1.5)) and np.array_equal(r, np.full(6, 0.5))
