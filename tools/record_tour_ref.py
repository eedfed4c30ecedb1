#!/usr/bin/env python3
"""Records tests/golden/tour_ref_cases.npz from the reference's own include/TSPSolver.hpp: random
cost maps of V = 2..13, 32 and 64 nodes in six kinds (entries in 0..5, so ties decide; asymmetric
entries in 0..999; symmetric ones; each of the three with 15 % INT_MAX off the diagonal), each run
through tools/record_tour_ref.cpp, which is compiled here against the reference header with an
empty <nlopt.hpp> on the include path (the reference includes it and uses nothing of it).  The
reference aborts where its nearest-neighbour search meets a row with no edge left: such a draw is
drawn again, up to TRIES times, and skipped after that.

  tools/record_tour_ref.py --ref <reference checkout> [--out tests/golden/tour_ref_cases.npz]

The fixture holds, per case k: m_k (V, V) int32, nn_k and opt_k (V,) int32, and `kinds`, the
cases' kind names.  No test runs this tool."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1
KINDS = ("ties", "asym", "sym", "ties_nopath", "asym_nopath", "sym_nopath")
SIZES = tuple(range(2, 14)) + (32, 64)
TRIES = 6


def draw(kind, V, rng):
    base = kind.split("_")[0]
    if base == "ties":
        m = rng.integers(0, 6, (V, V))
    elif base == "asym":
        m = rng.integers(0, 1000, (V, V))
    else:
        m = rng.integers(0, 1000, (V, V))
        m = np.triu(m, 1)
        m = m + m.T
    if kind.endswith("_nopath"):
        m[(rng.random((V, V)) < 0.15) & ~np.eye(V, dtype=bool)] = INT_MAX
    return m.astype(np.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ref", required=True, help="the reference checkout (its include/TSPSolver.hpp is compiled)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "tour_ref_cases.npz"))
    a = ap.parse_args()
    out, kinds, skipped = {}, [], 0
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "nlopt.hpp"), "w").close()
        exe = os.path.join(tmp, "record_tour_ref")
        subprocess.run(["g++", "-O2", "-std=c++17", "-w", "-I", tmp, "-I", os.path.join(a.ref, "include"), "-o", exe,
                        os.path.join(ROOT, "tools", "record_tour_ref.cpp")], check=True)
        for V in SIZES:
            for ki, kind in enumerate(KINDS):
                for t in range(TRIES):
                    m = draw(kind, V, np.random.default_rng([V, ki, t]))
                    r = subprocess.run([exe], input=f"{V}\n" + " ".join(map(str, m.reshape(-1))) + "\n",
                                       capture_output=True, text=True)
                    lines = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln[:2] in ("NN", "OP")}
                    if r.returncode == 0 and "NN" in lines and "OPT" in lines:
                        k = len(kinds)
                        out[f"m_{k}"] = m
                        out[f"nn_{k}"] = np.array(lines["NN"], np.int32)
                        out[f"opt_{k}"] = np.array(lines["OPT"], np.int32)
                        kinds.append(kind)
                        break
                else:
                    skipped += 1
    np.savez_compressed(a.out, kinds=np.array(kinds), **out)
    print(f"{len(kinds)} cases recorded, {skipped} (size, kind) pairs skipped after {TRIES} aborted draws -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
