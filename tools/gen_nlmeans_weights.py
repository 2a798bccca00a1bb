"""Writes savsr_amd/csrc/nlmeans_weights.hpp: the 577 literals of savsr_amd.nlmeans.WEIGHTS (the table's only definition) and one zero
behind them (index 577: every k >= 577), for csrc/nlmeans.hip.  tests/test_nlmeans.py pins the committed header to WEIGHTS entry by entry
and to this generator's text.

    python3 tools/gen_nlmeans_weights.py [--check]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from savsr_amd.nlmeans import N_WEIGHTS, WEIGHTS  # noqa: E402

PATH = os.path.join(ROOT, "savsr_amd", "csrc", "nlmeans_weights.hpp")


def text() -> str:
    vals = list(WEIGHTS) + [0]
    rows = [", ".join(f"{v:4d}" for v in vals[i:i + 16]) for i in range(0, len(vals), 16)]
    return ("// Written by tools/gen_nlmeans_weights.py from savsr_amd/nlmeans.py WEIGHTS: rint(4096 * exp(-i / 64)), i = 0 .. 576, then one 0\n"
            "// (index 577 stands for every k >= 577).  Do not edit: change WEIGHTS and run the generator.\n"
            "#pragma once\n#include <cstdint>\n\nnamespace savsr {\n\n"
            f"constexpr int NLM_N_WEIGHTS = {N_WEIGHTS};\n"
            f"constexpr uint16_t NLM_WEIGHTS[NLM_N_WEIGHTS + 1] = {{\n    " + ",\n    ".join(rows) + "};\n\n}  // namespace savsr\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare the committed header with the generator's text instead of writing it")
    a = ap.parse_args()
    if a.check:
        if open(PATH).read() != text():
            raise SystemExit(f"{PATH} differs from the generator's text")
        print("ok")
        return
    with open(PATH, "w") as f:
        f.write(text())
    print(PATH)


if __name__ == "__main__":
    main()
