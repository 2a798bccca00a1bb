"""Host-side memory check of csrc/pulldown.hip: its device functions, compiled unchanged into a stand-alone host program
(tools/host_check/) under -fsanitize=address,undefined, run one thread at a time over the tests' shapes, tile edges, offsets and ranges
on exact-size heap buffers and are compared with the numpy specification.  CPU only: nothing here is loaded into Python or run on a
GPU.  The host build takes the plain-C++ branches of the v_sad helpers (the builtins exist on the device only) and, because a launch
runs one thread at a time, the per-thread branch of the workgroup reduction (SAVSR_HOST_CHECK); everything else is the code the GPU runs.

    python3 tools/check_pulldown_host.py [--cxx /opt/rocm/llvm/bin/clang++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from savsr_amd.pulldown import field_scores, weave_matrix  # noqa: E402

HERE = os.path.join(ROOT, "tools", "host_check")
ORDERS = ("tff", "bff")


def build(cxx: str, work: str) -> str:
    src = open(os.path.join(ROOT, "savsr_amd", "csrc", "pulldown.hip")).read()
    assert src.count('#include "common.hpp"') == 1
    with open(os.path.join(work, "pulldown_device.inc"), "w") as f:
        f.write(src.replace('#include "common.hpp"', '#include "hip_stub.h"'))
    exe = os.path.join(work, "pulldown_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", work, "-I", HERE, "-I", os.path.join(ROOT, "savsr_amd", "csrc"),
                    os.path.join(HERE, "pulldown_main.cpp"), "-o", exe], check=True)
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "/opt/rocm/llvm/bin/clang++"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as work:
        exe = build(a.cxx, work)
        fin, fdelta, fout = (os.path.join(work, f) for f in ("in.bin", "delta.bin", "out.bin"))

        def frames_of(mats, wide, before, after):
            n = mats.shape[0]
            raw = mats.astype("<u2").view(np.uint8).reshape(n, -1) if wide else mats.reshape(n, -1)
            frames = rng.integers(0, 256, (n, before + raw.shape[1] + after), dtype=np.uint8)
            frames[:, before:before + raw.shape[1]] = raw
            return frames, raw.shape[1]

        def call(args):
            res = subprocess.run([exe] + [str(v) for v in args], capture_output=True, text=True)
            if res.returncode:
                raise SystemExit(f"FAILED {args}\n{res.stderr[-4000:]}")

        def scores(mats, depth, order, frm, to, before=0, after=0, mis=0):
            n, r, c = mats.shape
            frames, _ = frames_of(mats, depth != 8, before, after)
            frames.tofile(fin)
            args = [0 if depth == 8 else 1, n, frames.shape[1], before, r, c, depth, order, frm, to, 0, 0, mis, fin, fdelta, fout]
            call(args)
            got = np.fromfile(fout, dtype=np.int64).reshape(to - frm, 2)
            if not np.array_equal(got, field_scores(mats, ORDERS[order], depth)[frm:to]):
                raise SystemExit(f"MISMATCH {args}")

        def woven(mats, order, delta, frm, to, before=0, after=0, mis=0):
            n, r, c = mats.shape
            frames, pb = frames_of(mats, False, before, after)
            frames.tofile(fin)
            np.asarray(delta[frm:to], dtype=np.int32).tofile(fdelta)
            fb = frames.shape[1]
            args = [2, n, fb, before, r, c, 8, order, frm, to, fb, before, mis, fin, fdelta, fout]
            call(args)
            got = np.fromfile(fout, dtype=np.uint8).reshape(to - frm, fb)[:, before:before + pb].reshape(to - frm, r, c)
            if not np.array_equal(got, weave_matrix(mats, ORDERS[order], delta)[frm:to]):
                raise SystemExit(f"MISMATCH {args}")

        count = 0
        rows, widths = (1, 2, 3, 4, 5, 33), (1, 15, 16, 17, 256, 272, 319)
        for r in rows:
            for c in widths:
                for order in (0, 1):
                    for n in (1, 2, 3):
                        m = rng.integers(0, 256, (n, r, c), dtype=np.uint8)
                        delta = rng.integers(-1, 1, n).tolist()
                        for mis in (0, 1):
                            scores(m, 8, order, 0, n, mis=mis)
                            woven(m, order, delta, 0, n, mis=mis)
                            count += 2
                        m = rng.integers(0, 5000, (n, r, c)).astype(np.uint16)
                        for depth in (10, 12):
                            for mis in (0, 2):
                                scores(m, depth, order, 0, n, mis=mis)
                                count += 1
        for before, after in ((0, 0), (16, 16), (5, 3), (32, 0)):          # ranges with context, planes inside frames
            m = rng.integers(0, 256, (4, 9, 48), dtype=np.uint8)
            for order in (0, 1):
                for frm, to in ((0, 1), (1, 2), (1, 4), (3, 4), (2, 2)):
                    scores(m, 8, order, frm, to, before, after)
                    woven(m, order, [-1, -1, 0, -1], frm, to, before, after)
                    count += 2
                    if before % 2 == 0 and after % 2 == 0:
                        scores(rng.integers(0, 1024, (4, 9, 24)).astype(np.uint16), 10, order, frm, to, before, after)
                        count += 1
        tall = np.zeros((2, 2048, 64), dtype=np.uint8)          # the largest lane sums: 0 / 255 alternating by row parity
        tall[:, 1::2] = 255
        scores(tall, 8, 0, 0, 2)
        scores(tall, 8, 1, 0, 2, mis=1)
        count += 2
    print(f"ok: {count} cases equal the specification, no sanitizer report")


if __name__ == "__main__":
    main()
