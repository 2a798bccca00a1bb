"""Host-side memory check of the comb kernels (csrc/pulldown.hip `savsr_video_comb_windows_*`, csrc/deinterlace.hip
`savsr_video_deinterlace_masked_*`): their device functions, compiled unchanged into stand-alone host programs (tools/host_check/) under
-fsanitize=address,undefined, run one thread at a time over the tests' shapes, tile edges, offsets and ranges on exact-size heap buffers
and are compared with the numpy specification (savsr_amd/pulldown.py `comb_windows`; savsr_amd/deinterlace.py at rate "same" for the
flagged frames, a byte copy for the others).  CPU only: nothing here is loaded into Python or run on a GPU.  The host build takes the
plain-C++ branches of the v_sad helpers and, because a launch runs one thread at a time, the comb kernel's SAVSR_HOST_CHECK branch (the
LDS cells are a static array, the workgroup's last thread sums every lane's windows); everything else is the code the GPU runs.

    python3 tools/check_comb_host.py [--cxx /opt/rocm/llvm/bin/clang++]
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
from savsr_amd.pulldown import comb_windows  # noqa: E402

HERE = os.path.join(ROOT, "tools", "host_check")
ORDERS = ("tff", "bff")


def build(cxx: str, work: str, part: int) -> str:
    name = ("pulldown", "deinterlace")[part - 1]
    src = open(os.path.join(ROOT, "savsr_amd", "csrc", name + ".hip")).read()
    assert src.count('#include "common.hpp"') == 1
    with open(os.path.join(work, name + "_device.inc"), "w") as f:
        f.write(src.replace('#include "common.hpp"', '#include "hip_stub.h"'))
    exe = os.path.join(work, f"comb_host_{part}")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-DCOMB_PART={part}", "-I", work,
                    "-I", HERE, "-I", os.path.join(ROOT, "savsr_amd", "csrc"), os.path.join(HERE, "comb_main.cpp"), "-o", exe], check=True)
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "/opt/rocm/llvm/bin/clang++"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as work:
        exe_comb, exe_mask = build(a.cxx, work, 1), build(a.cxx, work, 2)
        fin, fflags, fout = (os.path.join(work, f) for f in ("in.bin", "flags.bin", "out.bin"))

        def frames_of(mats, wide, before, after):
            n = mats.shape[0]
            raw = mats.astype("<u2").view(np.uint8).reshape(n, -1) if wide else mats.reshape(n, -1)
            frames = rng.integers(0, 256, (n, before + raw.shape[1] + after), dtype=np.uint8)
            frames[:, before:before + raw.shape[1]] = raw
            return frames, raw.shape[1]

        def call(exe, args):
            res = subprocess.run([exe] + [str(v) for v in args], capture_output=True, text=True)
            if res.returncode:
                raise SystemExit(f"FAILED {args}\n{res.stderr[-4000:]}")

        def comb(mats, step, depth, order, frm, to, threshold=9, before=0, after=0, mis=0):
            n, r, c = mats.shape
            frames, _ = frames_of(mats, depth != 8, before, after)
            frames.tofile(fin)
            args = [8 if depth == 8 else 16, n, frames.shape[1], before, r, c, step if depth == 8 else depth, order, frm, to, 0, 0, mis, fin, fout, threshold]
            call(exe_comb, args)
            got = np.fromfile(fout, dtype=np.int64).reshape(to - frm, 2)
            want = comb_windows(mats, ORDERS[order], step, threshold, depth)[frm:to]
            if not np.array_equal(got, want):
                raise SystemExit(f"MISMATCH {args}: {got.tolist()} for {want.tolist()}")

        def masked(mats, step, depth, order, frm, to, method, flags, before=0, after=0, mis=0):
            n, r, c = mats.shape
            frames, pb = frames_of(mats, depth != 8, before, after)
            frames.tofile(fin)
            np.asarray(flags[frm:to], dtype=np.int32).tofile(fflags)
            fb = frames.shape[1]
            args = [8 if depth == 8 else 16, n, fb, before, r, c, step if depth == 8 else depth, order, frm, to, fb, before, mis, fin, fout, method, fflags]
            call(exe_mask, args)
            got = np.fromfile(fout, dtype=np.uint8).reshape(to - frm, fb)[:, before:before + pb]
            clean = (bwdif_matrix(mats, ORDERS[order], depth)[0] if method else deinterlace_matrix(mats, ORDERS[order], step, depth)[0])[0::2]
            want = np.where(np.asarray(flags, dtype=bool)[:, None, None], clean, mats)[frm:to]
            want = want.astype("<u2").view(np.uint8).reshape(to - frm, -1) if depth != 8 else want.astype(np.uint8).reshape(to - frm, -1)
            if not np.array_equal(got, want):
                raise SystemExit(f"MISMATCH {args}: {np.argwhere(got != want)[:5].tolist()}")

        count = 0
        # the comb windows: rows around the cell (8) and the tile (64 + 8 of halo), row bytes around the chunk (16), the cell (8 * step) and
        # the tile (512 + one cell)
        rows, widths = (2, 3, 4, 5, 9, 17, 33, 64, 65, 73, 130), (1, 7, 8, 9, 15, 16, 17, 33, 272, 319, 512, 528, 544, 1056)
        for r in rows:
            for c in widths:
                if r > 33 and c not in (17, 272, 528, 1056):
                    continue
                for order in (0, 1):
                    lo = rng.integers(0, 256, (2, 1, 1))          # (noise of a random spread: few, some or most samples combed)
                    m = ((rng.integers(0, 256, (2, r, c)) // int(rng.integers(1, 12)) + lo // 2) % 256).astype(np.uint8)
                    for step in (1, 2, 3, 4):
                        for mis in (0, 1):
                            comb(m, step, 8, order, 0, 2, threshold=int(rng.integers(0, 40)), mis=mis)
                            count += 1
                    if c <= 544:
                        w = rng.integers(0, 5000, (2, r, c)).astype(np.uint16)
                        for depth in (10, 12):
                            for mis in (0, 2):
                                comb(w, 1, depth, order, 0, 2, threshold=int(rng.integers(0, 40)), mis=mis)
                                count += 1
        for before, after in ((0, 0), (16, 16), (5, 3), (32, 0)):          # ranges with context, planes inside frames
            m = rng.integers(0, 256, (4, 19, 48), dtype=np.uint8)
            for order in (0, 1):
                for frm, to in ((0, 1), (1, 2), (1, 4), (3, 4), (2, 2)):
                    comb(m, 3, 8, order, frm, to, 9, before, after)
                    count += 1
                    if before % 2 == 0 and after % 2 == 0:
                        comb(rng.integers(0, 1024, (4, 19, 24)).astype(np.uint16), 1, 10, order, frm, to, 9, before, after)
                        count += 1
        full = np.zeros((2, 145, 1072), dtype=np.uint8)          # every second-field sample combed: the largest counts, several tiles each way
        full[:, 1::2] = 255
        comb(full, 1, 8, 0, 0, 2)
        comb(full, 1, 8, 1, 0, 2, mis=1)
        comb(full, 4, 8, 0, 0, 2, threshold=254)
        comb(full, 3, 8, 1, 0, 2, threshold=255)
        count += 4

        # the masked deinterlacer: both methods, both forms, every flag pattern, ranges with clamped neighbours
        for r, c in [(2, 1), (3, 1), (5, 7), (8, 16), (9, 33), (10, 32), (13, 48), (33, 272)]:
            for order in (0, 1):
                for n in (1, 2, 4):
                    m = rng.integers(0, 256, (n, r, c), dtype=np.uint8)
                    w = rng.integers(0, 5000, (n, r, c)).astype(np.uint16)
                    for flags in ([0] * n, [1] * n, [k % 2 for k in range(n)], [(k + 1) % 2 for k in range(n)]):
                        for method in (0, 1):
                            for mis in (0, 1):
                                masked(m, 1, 8, order, 0, n, method, flags, mis=mis)
                                masked(w, 1, (10, 12)[mis], order, 0, n, method, flags, mis=2 * mis)
                                count += 2
                        if c % 3 == 0:
                            masked(m, 3, 8, order, 0, n, 0, flags)
                            count += 1
        for before, after in ((0, 0), (16, 16), (5, 3), (32, 0)):
            m = rng.integers(0, 256, (4, 13, 48), dtype=np.uint8)
            for method in (0, 1):
                for frm, to in ((0, 1), (1, 2), (1, 4), (3, 4)):
                    masked(m, 3, 8, 0, frm, to, method, [1, 0, 1, 1], before, after)
                    masked(m, 1, 8, 1, frm, to, method, [0, 1, 1, 0], before, after)
                    count += 2
                    if before % 2 == 0 and after % 2 == 0:
                        masked(rng.integers(0, 1024, (4, 13, 24)).astype(np.uint16), 1, 10, 0, frm, to, method, [1, 1, 0, 1], before, after)
                        count += 1
    print(f"ok: {count} cases equal the specification, no sanitizer report")


if __name__ == "__main__":
    main()
