#!/usr/bin/env python3
"""Generates tests/golden/golden_neals.npz from the REFERENCE's own nmf_neals (TEST INFRASTRUCTURE ONLY; CPU only).

Run in the build container (needs /root/reference and oracle/_ref/libnmf_ref.so for the init stream):
    make -C oracle ref && python tests/golden/make_golden_neals.py

The reference's nmf_neals.c and its helpers are compiled where they lie into a temporary directory outside the tree,
with oracle/Makefile's flags and BLAS renames plus the LAPACK / BLAS routines nmf_neals.c needs, all onto scipy's
bundled OpenBLAS; the library is loaded with RTLD_LAZY.  Everything stored is data: inputs and the outputs the
reference produced for them.

The reference cannot return factors after an odd iteration count (it frees the caller's buffer, nmf_neals.c:432 / :477)
and frees one of the caller's buffers after an even one, so every buffer handed to it is malloc()ed here and never
freed by this script; factors are read back only after even counts.  The iteration count is always read.

Jobs (per-job scalars in the job_* arrays; job j's H as j{j}_H when the count is even, and its W as j{j}_W for the
FIXED jobs of seed 123: every W is one solve away from its H, and the file stays a few hundred KB.  W0 is not stored:
it is generateMatrix(ran)'s stream under srand(job_seed), which oracle/liboracle.so's init_restart restates bit for
bit -- asserted here for every job -- so the tests rebuild it from the seed):
  the bundled 1000 x 40 gct, k = 2..5, seeds 123..125 of the generateMatrix(ran) stream: FIXED 2, FIXED 10, and TolX = 1e-4
  with cap 2000;  a planted 300 x 70 matrix, k = 2..6, seeds 123..124: FIXED 2 and FIXED 4.
FIXED T is the reference run with cap T and TolX = TolFun = 0 (no test can fire).
A job is dropped (and printed) when the comparisons the tests make would not be robust for it: the long-double
restatement's count differs, delta at the stopping iteration or the one before lies within 1e-6 relative of TolX, or a
sample's two largest H entries differ by less than 1e-6 relative.  At most one job in six may be dropped.
"""
from __future__ import annotations

import ctypes
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import neals_ref  # noqa: E402
from pyoracle import Oracle, RefLib  # noqa: E402
from nmfconsensus_amd.synthetic import planted_matrix  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "golden_neals.npz")
SRCS = ["nmf_neals", "calculatenorm", "calculatemaxchange", "outputtiming"]
RENAMES = ["dgemm_", "dlange_", "dlamch_", "daxpy_", "dlacpy_", "dlaset_", "dnrm2_",   # oracle/Makefile's
           "dgesv_", "dgeqp3_", "dorgqr_", "dtrtrs_", "dcopy_", "dswap_"]
_dp = ctypes.POINTER(ctypes.c_double)
TOLX, CAP = 1e-4, 2000


def build_ref(td):
    import scipy
    blas = sorted(glob.glob(os.path.join(os.path.dirname(scipy.__file__) + ".libs", "libscipy_openblas-*.so")))[0]
    so = os.path.join(td, "libneals_ref.so")
    cmd = ["/opt/rocm/llvm/bin/clang", "-O2", "-g", "-fPIC", "-shared", "-ffp-contract=off",
           "-ftrivial-auto-var-init=zero", "-w", f"-I{REF}/libnmf/include", *[f"-D{r}=scipy_{r}" for r in RENAMES],
           *[f"{REF}/libnmf/{s}.c" for s in SRCS], "-o", so, blas, f"-Wl,-rpath,{os.path.dirname(blas)}", "-lm"]
    subprocess.run(cmd, check=True)
    L = ctypes.CDLL(so, mode=1)   # RTLD_LAZY
    ip = ctypes.POINTER(ctypes.c_int)
    L.nmf_neals.argtypes = [_dp, _dp, _dp, ip, ip, ip, ip, _dp, _dp]
    L.nmf_neals.restype = ctypes.c_double
    return L


libc = ctypes.CDLL(None)
libc.malloc.restype = ctypes.c_void_p
libc.malloc.argtypes = [ctypes.c_size_t]


def mbuf(arr):
    """A malloc()ed copy of arr (column-major), never freed here: (pointer, numpy view)."""
    flat = np.asarray(arr, dtype=np.float64).reshape(-1, order="F")
    p = libc.malloc(8 * max(flat.size, 1))
    view = np.ctypeslib.as_array(ctypes.cast(p, _dp), shape=(flat.size,))
    view[:] = flat
    return ctypes.cast(p, _dp), view


def run_ref(L, A, W0, cap, tolx, tolfun):
    m, n = A.shape
    k = W0.shape[1]
    pa, _ = mbuf(A)
    pw, vw = mbuf(W0)
    ph, vh = mbuf(np.zeros((k, n)))
    c = ctypes.c_int
    mi = c(cap)
    dn = L.nmf_neals(pa, pw, ph, ctypes.byref(c(m)), ctypes.byref(c(n)), ctypes.byref(c(k)), ctypes.byref(mi),
                     ctypes.byref(ctypes.c_double(tolx)), ctypes.byref(ctypes.c_double(tolfun)))
    it = mi.value
    W = H = None
    if it % 2 == 0:   # the caller's buffers hold the final factors (and were not freed) only after an even count
        W = vw.copy().reshape((m, k), order="F")
        H = vh.copy().reshape((k, n), order="F")
    return it, dn, W, H


def main():
    with np.load(os.path.join(HERE, "golden.npz")) as z:
        A_gct = np.asfortranarray(z["A_gct"])
    A_pl = planted_matrix(300, 70)
    ref = RefLib()
    orc = Oracle()
    jobs = []   # (matrix id, k, seed, mode, cap)
    for k in (2, 3, 4, 5):
        for seed in (123, 124, 125):
            jobs += [(0, k, seed, 0, 2), (0, k, seed, 0, 10), (0, k, seed, 1, CAP)]
    for k in (2, 3, 4, 5, 6):
        for seed in (123, 124):
            jobs += [(1, k, seed, 0, 2), (1, k, seed, 0, 4)]
    out = {}   # the matrices are not stored: golden.npz holds the gct, planted_matrix(300, 70) is the same on every host
    meta, dropped = [], []
    with tempfile.TemporaryDirectory() as td:
        L = build_ref(td)
        for mat, k, seed, mode, cap in jobs:
            A = A_gct if mat == 0 else A_pl
            W0, _ = ref.generate_ran(seed, A.shape[0], A.shape[1], k)
            assert np.array_equal(W0, orc.init_restart(seed, A.shape[0], A.shape[1], k)[0]), "init stream restatement"
            tolx = TOLX if mode else 0.0
            it, dn, W, H = run_ref(L, A, W0, cap, tolx, tolx)
            r = neals_ref.neals(A, W0, cap, TolX=tolx, TolFun=tolx, fixed=not mode, want_deltas=True)
            why = None
            if r["iters"] != it or r["status"] != 0:
                why = f"restatement count {r['iters']} status {r['status']} != reference {it}"
            elif mode and any(abs(d - tolx) <= 1e-6 * tolx for d in r["deltas"][-2:]):
                why = "delta within 1e-6 relative of TolX near the stop"
            else:
                s = np.sort(r["H"], axis=0)
                if np.any(s[-1] - s[-2] <= 1e-6 * np.abs(s[-1])):
                    why = "a sample's two largest H entries within 1e-6 relative"
            tag = f"mat={mat} k={k} seed={seed} mode={'tolx' if mode else 'fixed'} cap={cap} iters={it} dnorm={dn:.17g}"
            if why:
                dropped.append(tag + ": " + why)
                print("DROPPED", dropped[-1])
                continue
            j = len(meta)
            dist = -1.0
            if W is not None:
                out[f"j{j}_H"] = H
                if seed == 123 and not mode:
                    out[f"j{j}_W"] = W
                dist = max(np.linalg.norm(W - r["W"]) / np.linalg.norm(r["W"]),
                           np.linalg.norm(H - r["H"]) / np.linalg.norm(r["H"]))
                if mode:   # the restatement's H of a long job, so that the GPU test need not run it again
                    out[f"j{j}_Hld"] = r["H"]
            print(f"NEALS|golden|job {j}|{tag}|ref_dist={dist:.3e}")
            meta.append((mat, k, seed, mode, cap, it, dn, dist))
    assert 6 * len(dropped) <= len(jobs), f"{len(dropped)} of {len(jobs)} jobs dropped"
    mt = np.array(meta)
    out["job_mat"], out["job_k"], out["job_seed"] = mt[:, 0].astype(np.int32), mt[:, 1].astype(np.int32), mt[:, 2].astype(np.int32)
    out["job_tolx"], out["job_cap"], out["job_iters"] = mt[:, 3].astype(np.int32), mt[:, 4].astype(np.int32), mt[:, 5].astype(np.int32)
    out["job_dnorm"] = mt[:, 6].astype(np.float64)
    out["job_ref_dist"] = mt[:, 7].astype(np.float64)   # the reference's distance from the restatement; -1: odd count
    out["TolX"] = np.array(TOLX)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(meta), "jobs,", len(dropped), "dropped")


if __name__ == "__main__":
    main()
