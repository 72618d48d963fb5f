#!/usr/bin/env python3
"""Per-launch kernel times of the nmf_neals rule beside the nmf_mu rule, from one binary and one engine, interleaved.

    python tools/neals_kbench.py [--m 20000 --n 500 --kmin 2 --kmax 10 --R 200 --iters 20 --rounds 3]

Default: the C3 shape (20000 x 500, k = 2..10, R = 200), FIXED 20 iterations, every launch event-timed (set_timing).
Per rule and per round one line each for kernel id 1 (the H update: k_hupdate / k_hupdate_neals) and id 2 (the W side:
k_ahtw4, and under NEALS k_wsolve_neals behind it in the same timing scope), then the medians and the NEALS / MU ratio.
The figures of profiles/neals/README.md are this tool's output.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nmfconsensus_amd.nmf import Engine  # noqa: E402
from nmfconsensus_amd.synthetic import planted_matrix  # noqa: E402

KIDS = {0: "wta", 1: "hupdate", 2: "ahtw"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=20000)
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--kmin", type=int, default=2)
    ap.add_argument("--kmax", type=int, default=10)
    ap.add_argument("--R", type=int, default=200)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    A = planted_matrix(a.m, a.n)
    ks = list(range(a.kmin, a.kmax + 1))
    us = {(rule, kid): [] for rule in ("mu", "neals") for kid in KIDS}
    with Engine(A) as eng:
        eng.set_timing(True)
        for rnd in range(a.rounds + 1):   # round 0 warms up (buffers, code objects) and is not counted
            for rule in ("mu", "neals"):
                r = eng.run(ks, a.R, maxiter=a.iters, stop_rule=0, want_counts=False, neals=(rule == "neals"))
                info = eng.last_run_info()
                for kid, name in KIDS.items():
                    cnt, ms = eng.kernel_time(kid)
                    per = 1e3 * ms / max(cnt, 1)
                    if rnd:
                        us[(rule, kid)].append(per)
                    print(f"NEALS|kbench|round {rnd}|{rule}|{name}|launches {cnt}|{per:.1f} us per launch")
                print(f"NEALS|kbench|round {rnd}|{rule}|seconds_iterate {r.seconds_iterate:.4f}|"
                      f"ahtw_128 {info['ahtw_128']} ahtw_64 {info['ahtw_64']} ahtw_narrow {info['ahtw_narrow']}")
    for kid, name in KIDS.items():
        mu, ne = statistics.median(us[("mu", kid)]), statistics.median(us[("neals", kid)])
        print(f"NEALS|kbench|median|{name}|mu {mu:.1f} us|neals {ne:.1f} us|ratio {ne / mu:.3f}")


if __name__ == "__main__":
    main()
