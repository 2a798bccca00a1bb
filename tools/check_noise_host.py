"""Host-side memory check of csrc/noise.hip: its entries and device functions, compiled unchanged into a stand-alone host program
(tools/host_check/noise_main.cpp) under -fsanitize=address,undefined, run one thread at a time on exact-size heap buffers and compared
with the numpy specification (savsr_amd/noise.py `noise_stats_matrix`) on the shapes of tests/noise_cases.py.  CPU only: nothing here is
loaded into Python or run on a GPU.

What is covered.  The two entries with their refusals and the job they build; `ns_load` in its three forms (8 bytes and the dword behind
them, 16 bytes of 16-bit samples and the dword behind them, the single samples) and `ns_cell` (the two rows of second differences, the
column sums, the flat test, the bin) at steps 1 .. 4, depths 8 / 10 / 12 with samples above the top, progressive and field-wise with
odd row counts, planes without a cell, one workgroup plus ragged rests, planes whose last cell ends on the plane's last sample (the
frames end with the plane there, so a read beyond a cell's support is a sanitizer report), misaligned planes inside frames, several
frames, two calls adding into one table.  What is not: the host form runs the lanes one after the other and every lane adds its own
cell, so the LDS tables, their atomics and the barriers around them cannot show here; tests/test_gpu_noise.py covers those.

    python3 tools/check_noise_host.py [--cxx /opt/rocm/llvm/bin/clang++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from savsr_amd.noise import noise_stats_matrix  # noqa: E402
from tests.deblock_cases import as_bytes  # noqa: E402
from tests.noise_cases import SMALLEST, checkerboard, flat_beside_binned, stats_frames, stats_tile  # noqa: E402

HERE = os.path.join(ROOT, "tools", "host_check")


def build(cxx: str, work: str) -> str:
    src = open(os.path.join(ROOT, "savsr_amd", "csrc", "noise.hip")).read()
    assert src.count('#include "common.hpp"') == 1
    with open(os.path.join(work, "noise_device.inc"), "w") as f:
        f.write(src.replace('#include "common.hpp"', '#include "hip_stub.h"'))
    exe = os.path.join(work, "noise_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", work, "-I", HERE,
                    "-I", os.path.join(ROOT, "savsr_amd", "csrc"), os.path.join(HERE, "noise_main.cpp"), "-o", exe], check=True)
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "/opt/rocm/llvm/bin/clang++"))
    a = ap.parse_args()
    rng = np.random.default_rng(2)
    with tempfile.TemporaryDirectory() as work:
        exe = build(a.cxx, work)
        fin, fout = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")

        def call(args):
            return subprocess.run([exe] + [str(v) for v in args], capture_output=True, text=True)

        def stats(m, depth=8, interlaced=False, before=0, after=0, mis=0, calls=1):
            n, r, c, step = m.shape
            raw = as_bytes(m)
            fb = before + raw.shape[1] + after
            frames = rng.integers(0, 256, (n, fb), dtype=np.uint8)
            frames[:, before:before + raw.shape[1]] = raw
            frames.tofile(fin)
            args = [8 if depth == 8 else 16, n, fb, before, r, c, step, depth, int(interlaced), calls, mis, 0, fin, fout]
            res = call(args)
            if res.returncode:
                raise SystemExit(f"FAILED {args}\n{res.stderr[-4000:]}")
            got = np.fromfile(fout, dtype=np.int64).reshape(n, 256, 2)
            want = np.stack([sum(noise_stats_matrix(m[t, :, :, ch], depth, interlaced) for ch in range(step)) for t in range(n)]) * calls
            if not np.array_equal(got, want):
                raise SystemExit(f"MISMATCH {args}: {np.argwhere(got != want)[:5].tolist()}")

        count = 0
        for r, c in SMALLEST + ((1, 1), (2, 9), (19, 24), (20, 16), (21, 37), (35, 33), (26, 64)):
            for interlaced in (False, True):
                stats(stats_frames(rng, 1, r, c), 8, interlaced)
                count += 1
        tr, tc = stats_tile()
        for r, c in ((tr, tc), (tr + 5, tc + 6), (tr, tc + 14), (2 * tr + 3, 2 * tc + 4)):          # one workgroup; ragged rests; the vector form
            stats(stats_frames(rng, 1, r, c), 8, r % 2 == 1)
            count += 1
        for step in (1, 2, 3, 4):
            for depth, before, after, mis in ((8, 0, 0, 0), (8, 8, 0, 8), (8, 5, 3, 1), (10, 6, 2, 2), (10, 16, 0, 0), (12, 16, 0, 0)):
                cols = 48 if (before % 8 == 0 and mis % 8 == 0) else 37
                stats(stats_frames(rng, 3 if step == 1 else 1, 21, cols, step=step, depth=depth, above=True), depth, step == 3, before, after, mis)
                count += 1
        stats(checkerboard(26, 34)[None, :, :, None])
        stats(flat_beside_binned()[None, :, :, None])
        stats(np.full((1, 20, 24, 1), 200, np.uint8), interlaced=True)
        stats(stats_frames(rng, 3, 20, 32), 8, True, calls=2)          # frames do not leak into each other; calls add
        stats(stats_frames(rng, 2, 23, 24, depth=12, above=True), 12, True, 4, 2, 2, calls=2)
        count += 5
        # ---- the refusals: exit code 5, the entry named
        np.zeros(256, np.uint8).tofile(fin)
        ok = [8, 1, 64, 0, 8, 8, 1, 8, 0, 1, 0, 0, fin, fout]
        for slot, bad, words in ((1, 0, "n_frames >= 1"), (4, 0, "rows >= 1"), (5, 0, "at least one sample"), (6, 5, "step 1 .. 4"), (6, 0, "step 1 .. 4"),
                                 (2, 63, "frame_bytes smaller"), (3, -1, "plane offsets >= 0"), (11, 4, "8-byte aligned"), (8, 2, "interlaced 0 or 1"),
                                 (8, -1, "interlaced 0 or 1")):
            args = list(ok)
            args[slot] = bad
            res = call(args)
            if res.returncode != 5 or "video_noise_stats_u8" not in res.stderr or words not in res.stderr:
                raise SystemExit(f"REFUSAL {args}: exit {res.returncode}, {res.stderr[-400:]!r} (expected {words!r})")
            count += 1
        for args, words in (([16, 1, 128, 0, 8, 8, 1, 9, 0, 1, 0, 0, fin, fout], "depth 10 or 12"),
                            ([16, 1, 128, 0, 8, 8, 1, 10, 0, 1, 1, 0, fin, fout], "2-byte aligned"),
                            ([16, 1, 129, 0, 8, 8, 1, 10, 0, 1, 0, 0, fin, fout], "2-byte aligned")):
            res = call(args)
            if res.returncode != 5 or "video_noise_stats_u16" not in res.stderr or words not in res.stderr:
                raise SystemExit(f"REFUSAL {args}: exit {res.returncode}, {res.stderr[-400:]!r} (expected {words!r})")
            count += 1
    print(f"ok: {count} cases equal the specification or are refused by name, no sanitizer report")


if __name__ == "__main__":
    main()
