"""Build-level checks of the divergence kernels (CPU: compiles with hipcc, no GPU needed): k_br_div<K>, k_br_div_narrow
and k_br_div_sum keep no value in scratch and spill neither vector nor scalar registers, and the price of kernel id 3
(brunet.hip BR_LOG_OPS, the device log's VALU instructions) is the count in the ISA listing."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nmfconsensus_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_divergence_kernels_do_not_spill():
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-c",
                            os.path.join(CSRC, "brunet.hip"), "-o", os.path.join(td, "x.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for blk in r.stderr.split("Function Name: ")[1:]:
        name = blk.split()[0]
        if "k_br_div" not in name or "k_br_divide" in name:
            continue
        g = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
        seen[name] = dict(vspill=g("VGPRs Spill"), sspill=g("SGPRs Spill"), scratch=g(r"ScratchSize \[bytes/lane\]"),
                          occ=g(r"Occupancy \[waves/SIMD\]"), vgprs=g(r" VGPRs"))
    ranks = sorted(int(re.search(r"k_br_divILi(\d+)E", n).group(1)) for n in seen if "k_br_divILi" in n)
    assert ranks == list(range(2, 17)), ranks
    assert any("k_br_div_narrow" in n for n in seen) and any("k_br_div_sum" in n for n in seen)
    bad = {n: v for n, v in seen.items() if v["vspill"] or v["sspill"] or v["scratch"]}
    assert not bad, bad
    # at least four waves per SIMD at every rank (six for k <= 5)
    low = {n: v["occ"] for n, v in seen.items() if v["occ"] < 4}
    assert not low, low


def test_log_price_matches_the_isa_listing():
    """BR_LOG_OPS = the VALU instructions hipcc emits for one device log(double): everything between the load and the
    store of a one-line kernel but the moves of literals into registers and the address shift."""
    txt = open(os.path.join(CSRC, "brunet.hip")).read()
    ops = int(re.search(r"constexpr int BR_LOG_OPS = (\d+);", txt).group(1))
    with tempfile.TemporaryDirectory() as td:
        src, asm = os.path.join(td, "lg.hip"), os.path.join(td, "lg.s")
        with open(src, "w") as f:
            f.write("#include <hip/hip_runtime.h>\n"
                    "__global__ void k_lg(const double* x, double* y) { y[threadIdx.x] = log(x[threadIdx.x]); }\n")
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src, "-o", asm],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = open(asm).read().splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z4k_lg\w*:", l))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    valu = [l.split()[0] for l in lines[start:end] if re.match(r"^\s+v_", l)]
    valu = [o for o in valu if not o.startswith(("v_mov_b32", "v_lshlrev"))]
    assert len(valu) == ops, (len(valu), ops)
    hdr = open(os.path.join(ROOT, "include", "nmfc.h")).read()
    assert f"2k + 6 + {ops} lane-operations" in hdr
