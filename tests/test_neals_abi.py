"""The NEALS entry points at the ABI (CPU: no device work happens in any of these)."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_neals_symbols():
    from nmfconsensus_amd import _lib
    L = _lib.lib()
    out = os.popen(f"nm -D --defined-only {os.path.join(ROOT, 'nmfconsensus_amd', 'lib', 'libnmf.so')}").read()
    for name in ("nmf_neals", "nmfc_engine_set_neals", "nmfc_engine_neals_status"):
        assert hasattr(L, name), name
        assert f" T {name}\n" in out, name
        assert name in _lib.EXPORTED


@pytest.mark.parametrize("k", [1, 17])
def test_nmf_neals_rank_limit(capfd, k):
    """libnmf_compat.h: k outside 2..16 is refused before any device work, the factors untouched."""
    from nmfconsensus_amd import _lib
    rng = np.random.default_rng(0)
    a = np.asfortranarray(rng.random((40, 20)) + 0.1)
    w0, h0 = np.asfortranarray(rng.random((40, k))), np.asfortranarray(rng.random((k, 20)))
    w_in, h_in = w0.copy(), h0.copy()
    dp = ctypes.POINTER(ctypes.c_double)
    c = ctypes.c_int
    mi = c(100)
    ret = _lib.lib().nmf_neals(a.ctypes.data_as(dp), w0.ctypes.data_as(dp), h0.ctypes.data_as(dp), ctypes.byref(c(40)),
                               ctypes.byref(c(20)), ctypes.byref(c(k)), ctypes.byref(mi),
                               ctypes.byref(ctypes.c_double(1e-4)), ctypes.byref(ctypes.c_double(1e-4)))
    assert ret == -1 and mi.value == 100
    assert np.array_equal(w0, w_in) and np.array_equal(h0, h_in)
    assert f"Error in nmf_neals: k={k} unsupported (need 2 <= k <= 16)" in capfd.readouterr().err


def test_python_wrapper_rank_limit(capfd):
    from nmfconsensus_amd import libnmf
    rng = np.random.default_rng(1)
    a, w0, h0 = rng.random((30, 20)), rng.random((30, 17)), rng.random((17, 20))
    W, H, it, dn = libnmf.nmf_neals(a, w0, h0, 50)
    assert dn == -1 and it == 50 and np.array_equal(W, w0) and np.array_equal(H, h0)
    assert "k=17 unsupported" in capfd.readouterr().err


def test_set_neals_and_status_refuse_a_null_engine():
    from nmfconsensus_amd import _lib
    L = _lib.lib()
    assert L.nmfc_engine_set_neals(None, 1) == -1 and "no engine" in _lib.last_error()
    assert L.nmfc_engine_neals_status(None, None) == -1 and "no engine" in _lib.last_error()


def bare_engine(neals=False, euclid=None):
    """An Engine object with no device engine behind it: run() must raise on a bad combination before it touches one."""
    from nmfconsensus_amd.nmf import Engine
    eng = Engine.__new__(Engine)
    eng.h, eng.m, eng.n = None, 30, 20
    eng._neals, eng._euclid, eng._residuals = neals, euclid, False
    return eng


def test_run_refuses_neals_with_euclid():
    with pytest.raises(ValueError, match="exclude each other"):
        bare_engine().run([2], 1, neals=True, euclid=dict(stopconv=40, stopfreq=10))
    with pytest.raises(ValueError, match="exclude each other"):   # the engine's Euclidean setting is on
        bare_engine(euclid=dict(stopconv=40, stopfreq=10)).run([2], 1, neals=True)
    with pytest.raises(ValueError, match="exclude each other"):   # the engine's NEALS setting is on
        bare_engine(neals=True).run([2], 1, euclid=dict(stopconv=40, stopfreq=10))


def test_donmf_refuses_an_unknown_algorithm():
    from nmfconsensus_amd.nmf import doNMF, runNMFinJobs
    with pytest.raises(ValueError, match="algorithm"):
        doNMF(np.ones((4, 3)), 2, 10, algorithm="als")
    with pytest.raises(ValueError, match="algorithm"):
        runNMFinJobs(np.ones((4, 3)), [2], 1, 10, 123, algorithm="pg")
