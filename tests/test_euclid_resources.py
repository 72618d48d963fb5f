"""Compile-time guard of the Euclidean NMF() instantiations (CPU: compiles engine.hip with hipcc, no GPU needed).

The new rule lives in the epilogue of the A h^T tile and in the H-update kernel; the full-load A h^T form rests on three
workgroups per CU (3 waves per SIMD) like the form it derives from, so its registers are checked here, and
every form the engine launches in this mode must exist in engine.hip's translation unit without spills or scratch
(test_kernel_resources.py::test_no_register_spills sees them too).
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

# <GTG, NBUF, NPT, PR, WC, LATE, KHALF, RULE = 1>: GT and GT/2, each with and without the K-half skip, and the narrow tail
AHTW_EUCLID = ["k_ahtw4ILi128ELi2ELi1ELi64ELi4ELb1ELb0ELi1E", "k_ahtw4ILi128ELi2ELi1ELi64ELi4ELb1ELb1ELi1E",
               "k_ahtw4ILi64ELi2ELi1ELi64ELi4ELb1ELb0ELi1E", "k_ahtw4ILi64ELi2ELi1ELi64ELi4ELb1ELb1ELi1E",
               "k_ahtw4ILi32ELi3ELi1ELi16ELi2ELb0ELb0ELi1E"]
HUPD_EUCLID = "k_hupdateILi32ELi4ELi1E"
HUPD_MU = "k_hupdateILi32ELi4ELi0E"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_euclid_kernels_resources():
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

    for key in AHTW_EUCLID + [HUPD_EUCLID]:
        u = one(key)
        print(f"EUC|resources|{key}|{u}")
        assert u["spill"] == 0 and u["scratch"] == 0, (key, u)
    # the full-load form: 3 waves per SIMD, like k_ahtw4<GT, 2, 1, PANEL, 4, true, KHALF> with the nmf_mu rule
    for kh in "01":
        e, b = one(f"k_ahtw4ILi128ELi2ELi1ELi64ELi4ELb1ELb{kh}ELi1E"), one(f"k_ahtw4ILi128ELi2ELi1ELi64ELi4ELb1ELb{kh}ELi0E")
        assert e["occ"] >= 3 and e["occ"] >= b["occ"], (e, b)
    assert one(HUPD_EUCLID)["occ"] >= one(HUPD_MU)["occ"] >= 4
    # every form keeps the waves per SIMD of its nmf_mu counterpart: the epilogue's path for a block with a non-finite W0
    # (k_ahtw4, RULE_EUCLID) holds its loop-invariant values behind opaque copies so that it costs the hot path no
    # register; a compiler that undoes this shows here as a spill (above) or as lost occupancy
    for key in AHTW_EUCLID:
        e, b = one(key), one(key[:-4] + "Li0E")
        assert e["occ"] >= b["occ"], (key, e, b)
