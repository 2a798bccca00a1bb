"""Host-side memory check of csrc/scan.hip: its device functions, compiled unchanged into a stand-alone host program
(tools/host_check/) under -fsanitize=address,undefined, run one thread at a time over the tests' shapes, tile edges, misaligned bases,
lo / hi ranges and depths on exact-size heap buffers and are compared with the numpy specification (savsr_amd/scan.py `field_stats`).
CPU only: nothing here is loaded into Python or run on a GPU.  The host build takes the plain-C++ branches of the v_sad helpers (the
builtins exist on the device only) and, because a launch runs one thread at a time, the per-thread branch of the workgroup reduction
(SAVSR_HOST_CHECK); everything else is the code the GPU runs.

    python3 tools/check_scan_host.py [--cxx /opt/rocm/llvm/bin/clang++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from savsr_amd.scan import field_stats  # noqa: E402

HERE = os.path.join(ROOT, "tools", "host_check")


def build(cxx: str, work: str) -> str:
    src = open(os.path.join(ROOT, "savsr_amd", "csrc", "scan.hip")).read()
    assert src.count('#include "common.hpp"') == 1
    with open(os.path.join(work, "scan_device.inc"), "w") as f:
        f.write(src.replace('#include "common.hpp"', '#include "hip_stub.h"'))
    exe = os.path.join(work, "scan_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", work, "-I", HERE, "-I", os.path.join(ROOT, "savsr_amd", "csrc"),
                    os.path.join(HERE, "scan_main.cpp"), "-o", exe], check=True)
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "/opt/rocm/llvm/bin/clang++"))
    a = ap.parse_args()
    rng = np.random.default_rng(2)
    with tempfile.TemporaryDirectory() as work:
        exe = build(a.cxx, work)
        fin, fout = (os.path.join(work, f) for f in ("in.bin", "out.bin"))

        def stats(mats, depth=8, lo=0, hi=None, before=0, after=0, mis=0):
            n, r, c = mats.shape
            hi = n if hi is None else hi
            raw = mats.astype("<u2").view(np.uint8).reshape(n, -1) if depth != 8 else mats.reshape(n, -1)
            frames = rng.integers(0, 256, (n, before + raw.shape[1] + after), dtype=np.uint8)
            frames[:, before:before + raw.shape[1]] = raw
            frames.tofile(fin)
            args = [0 if depth == 8 else 1, n, frames.shape[1], before, r, c, depth, lo, hi, mis, fin, fout]
            res = subprocess.run([exe] + [str(v) for v in args], capture_output=True, text=True)
            if res.returncode:
                raise SystemExit(f"FAILED {args}\n{res.stderr[-4000:]}")
            got = np.fromfile(fout, dtype=np.int64).reshape(hi - lo, 8)
            if not np.array_equal(got, field_stats(mats, depth)[lo:hi]):
                raise SystemExit(f"MISMATCH {args}")
            return 1

        def u8(n, r, c):
            return rng.integers(0, 256, (n, r, c), dtype=np.uint8)

        def u16(n, r, c, top=5000):
            return rng.integers(0, top, (n, r, c)).astype(np.uint16)

        count = 0
        shapes = []
        # the GPU tests' shapes: packed [N, 9, 17, 1], [N, 7, 5, 3], [N, 12, 16, 3], [N, 3, 16, 1], [N, 2, 16, 1], [N, 5, 4112, 1], y400 8 x 32
        for r, c in ((9, 17), (7, 15), (12, 48), (3, 16), (2, 16), (5, 4112), (8, 32)):
            shapes.append(f"{r}x{c}")
            for n in (1, 2, 5):
                for mis in (0, 1):
                    count += stats(u8(n, r, c), mis=mis)
        # i420 6 x 10 at 8 bits: the Y plane in front of the chroma planes; i420 10 x 24 at 10 bits; i444 9 x 7 at 12 bits
        shapes += ["i420 6x10", "i420 10x24 @10", "i444 9x7 @12"]
        count += stats(u8(5, 6, 10), after=2 * 3 * 5)
        count += stats(u16(5, 10, 24, 1200), 10, after=2 * 2 * 5 * 12)
        count += stats(u16(5, 10, 24, 1200), 10, after=2 * 2 * 5 * 12, mis=2)
        count += stats(u16(5, 9, 7), 12, after=2 * 2 * 9 * 7)
        # every small row count and the widths around the 16-byte chunk and the workgroup's lanes, both depths
        rows, widths = (1, 2, 3, 4, 5, 7, 33), (1, 5, 15, 16, 17, 256, 272, 319)
        shapes.append(f"rows {rows} x widths {widths} at 8 / 10 / 12 bits")
        for r in rows:
            for c in widths:
                for n in (1, 2, 3):
                    for mis in (0, 1):
                        count += stats(u8(n, r, c), mis=mis)
                    m = u16(n, r, c)
                    for depth in (10, 12):
                        for mis in (0, 2):
                            count += stats(m, depth, mis=mis)
        # ranges with context, planes inside frames
        shapes.append("lo / hi ranges of 4 x 9x48 (8 bits) and 4 x 9x24 (10 bits) inside padded frames")
        for before, after in ((0, 0), (16, 16), (5, 3), (32, 0)):
            m = u8(4, 9, 48)
            for lo, hi in ((0, 1), (1, 2), (1, 4), (3, 4), (2, 2), (0, 4)):
                count += stats(m, 8, lo, hi, before, after)
                if before % 2 == 0 and after % 2 == 0:
                    count += stats(u16(4, 9, 24, 1024), 10, lo, hi, before, after)
        # the largest lane sums: 0 / 255 alternating by row parity and by frame
        tall = np.zeros((3, 2048, 64), dtype=np.uint8)
        tall[:, 1::2] = 255
        tall[1] = 255 - tall[1]
        shapes.append("3 x 2048x64 of 0 / 255")
        count += stats(tall)
        count += stats(tall, mis=1)
    print(f"ok: {count} cases equal the specification, no sanitizer report; shapes: {'; '.join(shapes)}")


if __name__ == "__main__":
    main()
