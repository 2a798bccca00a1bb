"""Host-side memory check of csrc/deinterlace.hip: its device functions, compiled unchanged into a stand-alone host program
(tools/host_check/) under -fsanitize=address,undefined, run one thread at a time over the tests' shapes on exact-size heap buffers and
are compared with the numpy specification -- the yadif entries, and the `_m` entries with both methods (yadif, bwdif against
`bwdif_matrix`) and both rates (double, same).  CPU only: nothing here is loaded into Python or run on a GPU.  The host build takes the
plain-C++ branch of `absdiff` (the v_sad builtins exist on the device only); everything else is the code the GPU runs.

    python3 tools/check_deinterlace_host.py [--cxx /opt/rocm/llvm/bin/clang++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from savsr_amd.deinterlace import bwdif_matrix, deinterlace_matrix  # noqa: E402

# R x C of tests/bwdif_cases.py: the smallest shapes at which bwdif's rule changes (no inner row, no line row, exactly one, both forms)
BWDIF_SHAPES = [(2, 1), (3, 1), (5, 7), (8, 16), (9, 33), (10, 32), (13, 48), (33, 272)]

HERE = os.path.join(ROOT, "tools", "host_check")


def build(cxx: str, work: str) -> str:
    src = open(os.path.join(ROOT, "savsr_amd", "csrc", "deinterlace.hip")).read()
    assert src.count('#include "common.hpp"') == 1
    with open(os.path.join(work, "deinterlace_device.inc"), "w") as f:
        f.write(src.replace('#include "common.hpp"', '#include "hip_stub.h"'))
    exe = os.path.join(work, "deinterlace_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", work, "-I", HERE, "-I", os.path.join(ROOT, "savsr_amd", "csrc"),
                    os.path.join(HERE, "deinterlace_main.cpp"), "-o", exe], check=True)
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "/opt/rocm/llvm/bin/clang++"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as work:
        exe = build(a.cxx, work)
        fin, fout = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")

        def run(kind, mats, step_or_depth, order, frm, to, before=0, after=0, mis=0, method=None, rate=0):
            """method None: the entries without a method; 0 / 1: the `_m` entries."""
            n, r, c = mats.shape
            raw = mats.astype("<u2").view(np.uint8).reshape(n, -1) if kind == 16 else mats.reshape(n, -1)
            fb = before + raw.shape[1] + after
            frames = rng.integers(0, 256, (n, fb), dtype=np.uint8)
            frames[:, before:before + raw.shape[1]] = raw
            frames.tofile(fin)
            args = [kind, n, fb, before, r, c, step_or_depth, order, frm, to, fb, before, mis, fin, fout] + ([] if method is None else [method, rate])
            res = subprocess.run([exe] + [str(v) for v in args], capture_output=True, text=True)
            if res.returncode:
                raise SystemExit(f"FAILED {args}\n{res.stderr[-4000:]}")
            out = np.fromfile(fout, dtype=np.uint8).reshape((1 if rate else 2) * (to - frm), fb)[:, before:before + raw.shape[1]]
            if method == 1:
                want = bwdif_matrix(mats, ("tff", "bff")[order], 8 if kind == 8 else step_or_depth)[0][2 * frm:2 * to]
            else:
                want = deinterlace_matrix(mats, ("tff", "bff")[order], step_or_depth if kind == 8 else 1, 8 if kind == 8 else step_or_depth)[0][2 * frm:2 * to]
            want = want[0::2] if rate else want
            want = want.astype("<u2").view(np.uint8).reshape(want.shape[0], -1) if kind == 16 else want.reshape(want.shape[0], -1)
            if not np.array_equal(out, want):
                raise SystemExit(f"MISMATCH {args}: {np.argwhere(out != want)[:5].tolist()}")

        count = 0
        shapes = [(2, 1), (3, 1), (2, 7), (5, 6), (5, 7), (9, 33), (31, 15), (32, 16), (33, 17), (33, 255), (32, 256), (34, 272), (65, 48), (4, 32)]
        for r, c in shapes:
            for order in (0, 1):
                for n in (1, 2, 3):
                    for step in (1, 2, 3, 4):
                        if c % step:
                            continue
                        m = rng.integers(0, 256, (n, r, c), dtype=np.uint8)
                        for mis in (0, 1):
                            run(8, m, step, order, 0, n, mis=mis)
                            count += 1
                    m = rng.integers(0, 5000, (n, r, c)).astype(np.uint16)
                    for depth in (10, 12):
                        for mis in (0, 2):
                            run(16, m, depth, order, 0, n, mis=mis)
                            count += 1
        for r, c in sorted(set(BWDIF_SHAPES + shapes)):          # the `_m` entries: bwdif at both rates, yadif at the same rate
            for order in (0, 1):
                for n in (1, 2, 3):
                    m = rng.integers(0, 256, (n, r, c), dtype=np.uint8)
                    w = rng.integers(0, 5000, (n, r, c)).astype(np.uint16)
                    if n == 3:          # a static frame run and hard edges: diff == 0, and the filters' overshoot into the clips
                        m[1], w[1] = m[0], w[0]
                        m[2, r // 2:], w[2, r // 2:] = 255, 4095
                    for rate in (0, 1):
                        for mis in (0, 1):
                            run(8, m, 1, order, 0, n, mis=mis, method=1, rate=rate)
                            run(16, w, (10, 12)[mis], order, 0, n, mis=2 * mis, method=1, rate=rate)
                            count += 2
                    run(8, m, 1, order, 0, n, method=0, rate=1)
                    run(8, m, 1, order, 0, n, mis=1, method=0, rate=0)
                    run(16, w, 10, order, 0, n, method=0, rate=1)
                    count += 3
        for before, after in ((0, 0), (16, 16), (5, 3), (32, 0)):          # ranges with context, planes inside frames
            m = rng.integers(0, 256, (3, 13, 48), dtype=np.uint8)
            for rate in (0, 1):
                run(8, m, 3, 0, 1, 2, before, after, method=1, rate=rate)
                run(8, m, 1, 1, 1, 3, before, after, method=1, rate=rate)
                run(8, m, 1, 1, 0, 1, before, after, method=0, rate=rate)
                count += 3
                if before % 2 == 0 and after % 2 == 0:
                    run(16, rng.integers(0, 1024, (3, 13, 24)).astype(np.uint16), 10, 0, 2, 3, before, after, method=1, rate=rate)
                    count += 1
            m = rng.integers(0, 256, (3, 9, 48), dtype=np.uint8)
            run(8, m, 3, 0, 1, 2, before, after)
            run(8, m, 1, 1, 1, 3, before, after)
            count += 2
            if before % 2 == 0 and after % 2 == 0:
                run(16, rng.integers(0, 1024, (3, 9, 24)).astype(np.uint16), 10, 0, 1, 2, before, after)
                count += 1
    print(f"ok: {count} cases equal the specification, no sanitizer report")


if __name__ == "__main__":
    main()
