"""Compile-time guard of the NEALS kernels (CPU: compiles engine.hip with hipcc, no GPU needed).

The rule took the two-kernel form (DESIGN.md "NEALS"): the A h^T tile's RULE_NEALS forms store the raw product and
k_wsolve_neals solves.  Every form the engine launches in this mode must exist in engine.hip's translation unit without
spills or scratch; the H kernel and each A h^T form keep at least the waves per SIMD of their nmf_mu counterparts; the
solve kernel is spill-free (test_kernel_resources.py::test_no_register_spills sees them all too).
"""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nmfconsensus_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# <GTG, NBUF, NPT, PR, WC, LATE, KHALF, RULE = 2>: GT and GT/2, each with and without the K-half skip, and the narrow tail
AHTW_NEALS = ["k_ahtw4ILi128ELi2ELi1ELi64ELi4ELb1ELb0ELi2E", "k_ahtw4ILi128ELi2ELi1ELi64ELi4ELb1ELb1ELi2E",
              "k_ahtw4ILi64ELi2ELi1ELi64ELi4ELb1ELb0ELi2E", "k_ahtw4ILi64ELi2ELi1ELi64ELi4ELb1ELb1ELi2E",
              "k_ahtw4ILi32ELi3ELi1ELi16ELi2ELb0ELb0ELi2E"]
HUPD_NEALS = "k_hupdate_neals"
HUPD_MU = "k_hupdateILi32ELi4ELi0E"
OTHERS = ["k_wsolve_neals", "k_neals_stop"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_neals_kernels_resources():
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-c",
                            os.path.join(CSRC, "engine.hip"), "-o", os.path.join(td, "x.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    use = {}
    for blk in r.stderr.split("Function Name: ")[1:]:
        g = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
        use[blk.split()[0]] = dict(spill=g("VGPRs Spill"), scratch=g(r"ScratchSize \[bytes/lane\]"),
                                   occ=g(r"Occupancy \[waves/SIMD\]"), vgprs=g("VGPRs"))

    def one(key):
        hits = [v for k, v in use.items() if key in k]
        assert len(hits) == 1, (key, [k for k in use if key in k])
        return hits[0]

    for key in AHTW_NEALS + [HUPD_NEALS] + OTHERS:
        u = one(key)
        print(f"NEALS|resources|{key}|{u}")
        assert u["spill"] == 0 and u["scratch"] == 0, (key, u)
    assert one(HUPD_NEALS)["occ"] >= one(HUPD_MU)["occ"] >= 4
    for key in AHTW_NEALS:
        e, b = one(key), one(key[:-4] + "Li0E")
        assert e["occ"] >= b["occ"], (key, e, b)
        assert e["vgprs"] <= b["vgprs"], (key, e, b)   # the epilogue holds neither W0 nor the h h^T rows
