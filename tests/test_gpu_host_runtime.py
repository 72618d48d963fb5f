"""The library's shared host runtime (csrc/nmfc_host.hpp) as the GPU entry points use it: launch timing changes no
result and no count, nmfc_nmf_mu_release() covers every arm of the nmf_mu drop-in, and a failed nmfc_brunet_create
leaves the process usable.  The parts that need no device run under the host sanitizers in
tests/test_host_sanitizers.py (tests/sanitize/host_runtime_driver.cpp)."""
import numpy as np
import pytest

from nmfconsensus_amd import _lib

pytestmark = pytest.mark.gpu

NOSTOP = 10 ** 6   # stopconv no restart reaches: fixed iteration count


def _same_run(a, b):
    assert len(a.W) == len(b.W)
    for x, y in zip(a.W + a.H, b.W + b.H):
        assert x.tobytes() == y.tobytes()
    for f in ("iters", "stopped_early", "labels", "counts", "consensus"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f


# nmfc_engine_kernel_time counts of test_engine_timing_changes_nothing's call by kernel id (WTA, HUPD, AHTW, INIT,
# OTHER, LABELS, COUNTS, SMALL, RESID), read off the library as it was before the host runtime was shared
ENGINE_COUNTS_STRIDE1 = [6, 6, 6, 1, 1, 1, 1, 0, 0]
ENGINE_COUNTS_STRIDE2 = [3, 3, 3, 1, 1, 1, 1, 0, 0]


@pytest.mark.parametrize("stride", [1, 2])
def test_engine_timing_changes_nothing(monkeypatch, stride):
    """MU engine, (130, 17), k = 2, 3, R = 3, FIXED 6 iterations on the general path (NMFC_SMALL=0): timing off, on
    (every stride-th iteration), off again on one engine give the same bytes; nmfc_engine_kernel_time counts the
    drained event pairs -- with stride 1 every launch of the run (the literals are what this call launches: one init,
    six iterations of three kernels, one move when the live panels are archived, one labels and one counts pass),
    with stride 2 the iteration kernels of iterations 2, 4, 6 -- and nothing when timing is off."""
    from nmfconsensus_amd.nmf import Engine
    monkeypatch.setenv("NMFC_SMALL", "0")
    rng = np.random.default_rng(13017)
    A = np.asfortranarray(rng.random((130, 17)) + 0.1)
    kids = (_lib.KID_WTA, _lib.KID_HUPD, _lib.KID_AHTW, _lib.KID_INIT, _lib.KID_OTHER, _lib.KID_LABELS,
            _lib.KID_COUNTS, _lib.KID_SMALL, _lib.KID_RESID)
    expect = {1: ENGINE_COUNTS_STRIDE1, 2: ENGINE_COUNTS_STRIDE2}[stride]
    with Engine(A) as eng:
        runs = []
        for on in (False, True, False):
            eng.set_timing(on, stride)
            runs.append(eng.run([2, 3], 3, maxiter=6, seed=11, stop_rule=_lib.STOP_FIXED, want_factors=True))
            got = [eng.kernel_time(k) for k in kids]
            print(f"HOSTRT|engine|stride {stride}|timing {on}|(count, ms) per kid {got}")
            if on:
                assert [c for c, _ in got] == expect
                assert all((ms > 0) == (c > 0) for c, ms in got)
            else:
                assert all(c == 0 and ms == 0 for c, ms in got)
    assert all(int(t) == 6 for t in runs[0].iters)
    _same_run(runs[0], runs[1])
    _same_run(runs[0], runs[2])


@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("m,n,ks", [(64, 5, [2]), (129, 37, [2, 3])])
def test_brunet_timing_changes_nothing(m, n, ks, lanes):
    """Brunet engine, B = 3 restarts, 20 iterations, nothing stops: timing off, on, off on one engine give the same
    bytes; nmfc_brunet_kernel_time counts every launch, nk x 20 per iteration kernel, timed or not, and accumulates
    event time only while timing is on."""
    from nmfconsensus_amd.brunet import BrunetEngine
    rng = np.random.default_rng(1000 * m + n)
    A = np.asfortranarray(rng.random((m, n)) * 3.0 + 0.05)
    kids = (_lib.BK_HNUM, _lib.BK_HUPD, _lib.BK_WUPD)
    with BrunetEngine(A) as eng:
        runs = []
        for on in (False, True, False):
            eng.set_timing(on)
            runs.append(eng.run(ks, 3, maxiter=20, seed=77, stopconv=NOSTOP, lanes=lanes, want_factors=True))
            got = [eng.kernel_time(k) for k in kids]
            print(f"HOSTRT|brunet|{m}x{n}|lanes {lanes}|timing {on}|(count, ms, flop) per kid {got}")
            for cnt, ms, _ in got:
                assert cnt == len(ks) * 20
                assert ms > 0 if on else ms == 0
    assert all(int(t) == 20 for t in runs[0].iters)
    _same_run(runs[0], runs[1])
    _same_run(runs[0], runs[2])


def test_nmf_mu_release_covers_every_arm(golden, monkeypatch):
    """One nmf_mu call on each arm of the drop-in on the gct -- generic (k = 20), solo (k = 2), team (k = 9,
    NMFC_SOLO=0) and the batched engine with a batch of one (k = 9, NMFC_SMALL=0) -- then nmfc_nmf_mu_release() twice
    in a row, then each arm again: the second round equals the first byte for byte.  (Whether the release frees the
    generic arm's device memory is checked by reading generic.hip: free device memory moves under other work on a
    shared GPU, so no test asserts on it.)"""
    from nmfconsensus_amd import libnmf
    L = _lib.lib()
    A = golden["A_gct"]
    m, n = A.shape
    rng = np.random.default_rng(209)
    init = {k: (rng.uniform(0.1, 1.0, (m, k)), rng.uniform(0.1, 1.0, (k, n))) for k in (20, 9)}
    init[2] = (golden["init_k2_W"], golden["init_k2_H"])
    arms = (("generic", 20, {}), ("solo", 2, {}), ("team", 9, {"NMFC_SOLO": "0"}),
            ("batch of one", 9, {"NMFC_SOLO": "0", "NMFC_SMALL": "0"}))
    assert L.nmfc_mu_solo_fits(m, n, 2)

    def one_round():
        out = []
        for _, k, env in arms:
            with monkeypatch.context() as mp:
                for name, v in env.items():
                    mp.setenv(name, v)
                out.append(libnmf.nmf_mu(A, *init[k], 40))
        return out

    L.nmfc_nmf_mu_release()
    first = one_round()
    L.nmfc_nmf_mu_release()
    L.nmfc_nmf_mu_release()
    second = one_round()
    L.nmfc_nmf_mu_release()   # later tests get an engine made under their own environment
    for (name, k, _), a, b in zip(arms, first, second):
        assert a["ret"] == 0 and b["ret"] == 0 and a["maxiter"] == b["maxiter"], name
        assert a["w0"].tobytes() == b["w0"].tobytes() and a["h0"].tobytes() == b["h0"].tobytes(), name
        assert a["w0"].tobytes() != np.asfortranarray(init[k][0]).tobytes(), name   # the arm wrote its factors


def test_failed_brunet_create_leaves_usable_process():
    """nmfc_brunet_create refuses a matrix with a negative entry and one with an entry above 2^64 (NULL, "finite,
    non-negative"), freeing what it had allocated on the way; a create + run on the valid matrix straight afterwards
    gives the bytes of a run before the failures."""
    from nmfconsensus_amd.brunet import BrunetEngine
    rng = np.random.default_rng(645)
    A = np.asfortranarray(rng.random((64, 5)) * 3.0 + 0.05)

    def run():
        with BrunetEngine(A) as eng:
            return eng.run([2, 3], 3, maxiter=20, seed=5, stopconv=NOSTOP, want_factors=True)

    before = run()
    for bad in (-1.0, np.nextafter(2.0 ** 64, np.inf)):
        B = A.copy(order="F")
        B[41, 3] = bad
        with pytest.raises(RuntimeError, match="finite, non-negative"):
            BrunetEngine(B)
    _same_run(before, run())
