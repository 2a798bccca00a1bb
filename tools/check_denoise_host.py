"""Host-side memory check of csrc/denoise.hip: its device functions, compiled unchanged into a stand-alone host program
(tools/host_check/) under -fsanitize=address,undefined, run one thread at a time on exact-size heap buffers and are compared with the
numpy specification (savsr_amd/denoise.py `denoise_matrix`): both forms (planes whose bytes are a multiple of 16 on aligned bases, and
everything else), misaligned bases, planes inside frames, every radius of the tests, videos shorter than the radius, and from / to
sub-ranges whose taps lie outside them.  CPU only: nothing here is loaded into Python or run on a GPU.  The host build votes per
thread where the GPU votes per wave (a lane whose walks have ended leaves the loop on its own); everything else is the code the GPU runs.

    python3 tools/check_denoise_host.py [--cxx /opt/rocm/llvm/bin/clang++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from savsr_amd.denoise import denoise_matrix  # noqa: E402
from tests.denoise_cases import MATRICES, RADII, STRENGTH, TIGHT, as_bytes, lengths_for, walk_video  # noqa: E402

HERE = os.path.join(ROOT, "tools", "host_check")


def build(cxx: str, work: str) -> str:
    src = open(os.path.join(ROOT, "savsr_amd", "csrc", "denoise.hip")).read()
    assert src.count('#include "common.hpp"') == 1
    with open(os.path.join(work, "denoise_device.inc"), "w") as f:
        f.write(src.replace('#include "common.hpp"', '#include "hip_stub.h"'))
    exe = os.path.join(work, "denoise_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", work, "-I", HERE,
                    "-I", os.path.join(ROOT, "savsr_amd", "csrc"), os.path.join(HERE, "denoise_main.cpp"), "-o", exe], check=True)
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "/opt/rocm/llvm/bin/clang++"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as work:
        exe = build(a.cxx, work)
        fin, fout = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")

        def run(mats, depth, radius, strength, frm, to, before=0, after=0, mis=0):
            n, r, c = mats.shape
            raw = as_bytes(mats)
            fb = before + raw.shape[1] + after
            frames = rng.integers(0, 256, (n, fb), dtype=np.uint8)
            frames[:, before:before + raw.shape[1]] = raw
            frames.tofile(fin)
            args = [8 if depth == 8 else 16, n, fb, before, r, c, depth, radius, strength[0], strength[1], frm, to, fb, before, mis, fin, fout]
            res = subprocess.run([exe] + [str(v) for v in args], capture_output=True, text=True)
            if res.returncode:
                raise SystemExit(f"FAILED {args}\n{res.stderr[-4000:]}")
            got = np.fromfile(fout, dtype=np.uint8).reshape(to - frm, fb)
            want = as_bytes(denoise_matrix(mats, radius, *strength, depth)[frm:to])
            if not np.array_equal(got[:, before:before + raw.shape[1]], want):
                raise SystemExit(f"MISMATCH {args}: {np.argwhere(got[:, before:before + raw.shape[1]] != want)[:5].tolist()}")
            if not (np.all(got[:, :before] == 0xA5) and np.all(got[:, before + raw.shape[1]:] == 0xA5)):
                raise SystemExit(f"WROTE OUTSIDE THE PLANE {args}")

        count = 0
        for r, c in MATRICES:
            for radius in RADII:
                for n in lengths_for(radius):
                    for depth in (8, 10, 12):
                        m = walk_video(rng, n, r, c, depth)
                        step = 1 if depth == 8 else 2
                        for mis in (0, step):
                            run(m, depth, radius, STRENGTH, 0, n, mis=mis)
                            count += 1
                        if radius <= 2:
                            run(m, depth, radius, TIGHT, 0, n)
                            count += 1
        for before, after in ((0, 0), (16, 16), (6, 2), (32, 0)):          # planes inside frames; sub-ranges with their taps outside
            for radius in (2, 4):
                n = 2 * radius + 6
                for r, c in ((4, 32), (5, 33)):
                    for depth in (8, 12):
                        m = walk_video(rng, n, r, c, depth)
                        for frm, to in ((0, 1), (radius, radius + 3), (n - 2, n), (1, n - 1)):
                            run(m, depth, radius, STRENGTH, frm, to, before, after)
                            count += 1
        for depth in (8, 10, 12):          # the top of the range: every k at the largest sums; samples above the depth's range are clipped
            top = (1 << depth) - 1
            for n in list(range(1, 17)) + [38]:          # (n frames of one value at radius 16: k = n up to 17, then 17 .. 33)
                run(np.full((n, 2, 32 if n % 2 else 5), top, dtype=np.uint8 if depth == 8 else np.uint16), depth, 16, (255, 255), 0, n)
                count += 1
            if depth != 8:
                run(np.full((5, 2, 8), 0xFFFF, dtype=np.uint16), depth, 2, STRENGTH, 0, 5)
                run(np.full((5, 1, 3), 0xFFFF, dtype=np.uint16), depth, 2, STRENGTH, 0, 5)
                count += 2
    print(f"ok: {count} cases equal the specification, no sanitizer report")


if __name__ == "__main__":
    main()
