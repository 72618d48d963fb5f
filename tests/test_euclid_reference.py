"""The numpy restatement of the BROAD script's Euclidean NMF() (tests/euclid_ref.py) checked against itself on the CPU:
its stop rule's corner cases, the monotone residual, the Gram form against the long-double literal form, and -- the
condition that makes test_gpu_euclid.py's iteration-count comparison meaningful -- that the literal and the Gram fp64
forms stop at the same iteration with the same labels on every input that test uses.
"""
import numpy as np
import pytest

import euclid_ref as er
from conftest import relfro

LD = np.longdouble


def small_case(m=97, n=33, k=3, seed=31):
    V = er.planted(m, n)
    W0, H0 = er.r_init(seed, m, n, k)
    return V, W0, H0


def test_first_check_never_counts():
    """old.membership starts at 0 and classes are 1-based, so the check at t = stopfreq always sees a change."""
    V, W0, H0 = small_case()
    for stopfreq in (1, 3, 10):
        trace = []
        er.run(V, W0, H0, 4 * stopfreq, stopconv=1000, stopfreq=stopfreq, trace=trace)
        assert trace[0] == (stopfreq, 0), trace[:2]
        assert [t for t, _ in trace] == [stopfreq * (i + 1) for i in range(4)]


def test_earliest_stop():
    """stopconv = 1, stopfreq = 1 stops at t = 2 at the earliest; in general not before (stopconv + 1) stopfreq."""
    V, W0, H0 = small_case()
    for form in ("literal", "gram"):
        _, _, t, early = er.run(V, W0, H0, 500, stopconv=1, stopfreq=1, form=form)
        assert early == 1 and t >= 2
        _, _, t, early = er.run(V, W0, H0, 2000, stopconv=5, stopfreq=3, form=form)
        assert early == 1 and t >= 18 and t % 3 == 0
    _, _, t, early = er.run(V, W0, H0, 17, stopconv=5, stopfreq=3)
    assert (t, early) == (17, 0)
    # the rule firing at t = maxiter still reports an early stop
    _, _, t_stop, _ = er.run(V, W0, H0, 2000, stopconv=5, stopfreq=3)
    _, _, t, early = er.run(V, W0, H0, t_stop, stopconv=5, stopfreq=3)
    assert (t, early) == (t_stop, 1)


def test_fixed_runs_maxiter():
    V, W0, H0 = small_case()
    _, _, t, early = er.run(V, W0, H0, 37, stopconv=1, stopfreq=1, fixed=True)
    assert (t, early) == (37, 0)


@pytest.mark.parametrize("form", ["literal", "gram"])
def test_residual_does_not_increase(form):
    """The Frobenius MU update never increases ||V - W H||_F; the + eps and the fp64 roundings of the factors move
    W H by at most a few eps (|W||H|) per element, so the slack is 64 eps (||V||_F + ||W||_F ||H||_F)."""
    V, W0, H0 = small_case(130, 17, 5, seed=77)
    keep = {t: None for t in range(1, 41)}
    er.run(V, W0, H0, 40, form=form, fixed=True, keep=keep)
    prev = er.frob(V, W0, H0)
    for t in range(1, 41):
        W, H = keep[t]
        cur = er.frob(V, W, H)
        slack = 64 * er.EPS * (np.linalg.norm(V) + np.linalg.norm(W) * np.linalg.norm(H))
        assert cur <= prev + slack, (t, cur, prev)
        prev = cur
    assert prev < 0.5 * er.frob(V, W0, H0)


@pytest.mark.parametrize("m,n,k", [(97, 33, 3), (130, 17, 2), (130, 17, 5)])
def test_gram_form_matches_long_double_literal(m, n, k):
    """The engine's form of the denominators, in fp64, against the script's form in long double after 30 iterations:
    far inside the 1e-9 the GPU test allows (printed)."""
    V, W0, H0 = small_case(m, n, k, seed=500 + k)
    Wl, Hl, _, _ = er.run(V, W0, H0, 30, form="literal", dtype=LD, fixed=True)
    Wg, Hg, _, _ = er.run(V, W0, H0, 30, form="gram", fixed=True)
    ew, eh = relfro(Wg, Wl.astype(np.float64)), relfro(Hg, Hl.astype(np.float64))
    print(f"EUC|gram fp64 vs literal long double|{m}x{n} k={k}|W {ew:.3g}|H {eh:.3g}")
    assert ew <= 1e-12 and eh <= 1e-12
    assert np.all(Wg >= er.EPS) and np.all(Hg >= er.EPS)


@pytest.mark.parametrize("shape", list(er.STOP_SHAPES))
@pytest.mark.parametrize("setting", er.STOP_SETTINGS)
def test_literal_and_gram_forms_stop_alike(shape, setting):
    """Every job of the GPU stop-rule test (R-stream inits): the same iteration count, early flag and labels from the
    literal and the Gram fp64 forms, except the jobs named in euclid_ref.STOP_EXCLUDED (at most one)."""
    assert len(er.STOP_EXCLUDED) <= 1
    g = er.stop_reference(shape, setting, "gram")
    l = er.stop_reference(shape, setting, "literal")
    assert set(g) == {(k, i) for k in er.STOP_KS for i in range(1, er.STOP_R + 1)}
    bad = [key for key in g if (shape, setting) + key not in er.STOP_EXCLUDED and
           (g[key][0] != l[key][0] or g[key][1] != l[key][1] or not np.array_equal(g[key][2], l[key][2]))]
    ts = [v[0] for v in g.values()]
    print(f"EUC|stop|{shape}|{setting}|t {min(ts)}..{max(ts)}|early {sum(v[1] for v in g.values())}/{len(g)}")
    assert not bad, bad
    # the set exercises the rule: every job stops by it, none before the first possible check
    assert all(v[1] == 1 and v[0] >= (setting[0] + 1) * setting[1] for v in g.values())
