"""Host-side memory check of csrc/nlmeans.hip: its device code, compiled unchanged into a stand-alone host program (tools/host_check/)
under -fsanitize=address,undefined, run one thread at a time on exact-size heap buffers and compared with the numpy specification
(savsr_amd/nlmeans.py `nlm_matrix`) on the shapes of tests/nlmeans_cases.py: planes smaller than the halo, one tile plus a row and a
column, every patch x search, the divisor's range, every depth with samples above it, the largest numerator, a plane of 0xFFFF, steps 1
and 3, 1 and 3 frames, planes inside frames at misaligned bases.  CPU only: nothing here is loaded into Python or run on a GPU.

What is covered: the two entries with their refusals and the job they build (the magic multiplier of the division by D), and the device
functions every form shares -- `nlm_sample` (the clamped, stepped read, also what the tiled kernel stages its LDS tile with),
`nlm_bucket` (shift, multiply-shift division, the clamp to 577), the weight table, `nlm_mean` and `nlm_store` -- driven by the host
form of `nlm_tile_kernel`, in which a lane owns one output sample and evaluates every patch term from memory.  What is not: the tiled
kernel itself.  It cannot be driven one thread at a time (a workgroup shares the LDS tile behind a barrier and a wave sums columns with
DPP shifts), so its LDS indexing, its register rings and its cross-lane sums are covered by tests/test_gpu_nlmeans.py alone.

    python3 tools/check_nlmeans_host.py [--cxx /opt/rocm/llvm/bin/clang++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from savsr_amd.nlmeans import divisor, nlm_matrix  # noqa: E402
from tests.nlmeans_cases import DEPTHS, MAX_DIVISOR, PATCHES, SEARCHES, TINY, as_bytes, case_frames, one_tile_plus  # noqa: E402

HERE = os.path.join(ROOT, "tools", "host_check")


def build(cxx: str, work: str) -> str:
    src = open(os.path.join(ROOT, "savsr_amd", "csrc", "nlmeans.hip")).read()
    assert src.count('#include "common.hpp"') == 1
    with open(os.path.join(work, "nlmeans_device.inc"), "w") as f:
        f.write(src.replace('#include "common.hpp"', '#include "hip_stub.h"'))
    exe = os.path.join(work, "nlmeans_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", work, "-I", HERE,
                    "-I", os.path.join(ROOT, "savsr_amd", "csrc"), os.path.join(HERE, "nlmeans_main.cpp"), "-o", exe], check=True)
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "/opt/rocm/llvm/bin/clang++"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as work:
        exe = build(a.cxx, work)
        fin, fout = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")

        def run(m, depth, patch, search, div, before=0, after=0, mis=0):
            n, r, c, step = m.shape
            raw = as_bytes(m)
            fb = before + raw.shape[1] + after
            frames = rng.integers(0, 256, (n, fb), dtype=np.uint8)
            frames[:, before:before + raw.shape[1]] = raw
            frames.tofile(fin)
            args = [8 if depth == 8 else 16, n, fb, before, r, c, step, depth, patch, search, div, fb, before, mis, fin, fout]
            res = subprocess.run([exe] + [str(v) for v in args], capture_output=True, text=True)
            if res.returncode:
                raise SystemExit(f"FAILED {args}\n{res.stderr[-4000:]}")
            got = np.fromfile(fout, dtype=np.uint8).reshape(n, fb)
            want = np.empty_like(m)
            for t in range(n):
                for ch in range(step):
                    want[t, :, :, ch] = nlm_matrix(m[t, :, :, ch], depth, patch, search, div)
            if not np.array_equal(got[:, before:before + raw.shape[1]], as_bytes(want)):
                raise SystemExit(f"MISMATCH {args}: {np.argwhere(got[:, before:before + raw.shape[1]] != as_bytes(want))[:5].tolist()}")
            if not (np.all(got[:, :before] == 0xA5) and np.all(got[:, before + raw.shape[1]:] == 0xA5)):
                raise SystemExit(f"WROTE OUTSIDE THE PLANE {args}")

        count = 0
        for patch in PATCHES:
            for search in SEARCHES:
                for r, c in TINY:
                    run(case_frames(rng, 1, r, c), 8, patch, search, divisor(patch, 3.0))
                    count += 1
                run(case_frames(rng, 1, 17, 9, depth=10, above=True), 10, patch, search, divisor(patch, 3.0), mis=2)
                count += 1
        run(case_frames(rng, 1, *one_tile_plus(3)), 8, 3, 3, divisor(3, 3.0))          # (search 3: the host form pays every patch term)
        count += 1
        for depth in DEPTHS:
            m = case_frames(rng, 1, 12, 20, depth=depth, above=True)
            for div in (1, divisor(3, 3.0), MAX_DIVISOR):
                run(m, depth, 3, 7, div)
                count += 1
        run(np.full((1, 17, 20, 1), 4095, np.uint16), 12, 3, 7, 441)          # the largest numerator: 225 * 4096 * 4095
        run(np.full((1, 5, 8, 1), 0xFFFF, np.uint16), 10, 3, 7, 441)
        run(np.full((1, 5, 8, 1), 0xFFFF, np.uint16), 12, 2, 3, 1)
        count += 3
        for step in (1, 3):          # steps, frames, planes inside frames at misaligned bases
            for n in (1, 3):
                for depth, before, after, mis in ((8, 0, 0, 0), (8, 5, 3, 1), (12, 6, 2, 2)):
                    run(case_frames(rng, n, 9, 11, step=step, depth=depth, above=True), depth, 2, 3, divisor(2, 3.0), before, after, mis)
                    count += 1
    print(f"ok: {count} cases equal the specification, no sanitizer report")


if __name__ == "__main__":
    main()
