"""Host-side memory check of csrc/deblock.hip: its entries and device functions, compiled unchanged into a stand-alone host program
(tools/host_check/) under -fsanitize=address,undefined, run one thread at a time on exact-size heap buffers and compared with the numpy
specification (savsr_amd/deblock.py `deblock_matrix` / `deblock_fields`) on the shapes of tests/deblock_cases.py: planes with no edge,
the plane whose only edge is its last sample, one tile plus a row and a column, two tiles each way with a ragged rest, blocks 4 / 8 / 16
in both modes, progressive and field-wise with odd row counts, every depth with samples above it, thresholds (0, 0), the defaults and
(255, 255) on noise, steps 1 .. 4, 1 and 3 frames, planes inside frames at misaligned bases, and the entries' refusals.  CPU only:
nothing here is loaded into Python or run on a GPU.

What is covered: the two entries with their refusals and the job they build, and the four phases of the tiled kernel as the GPU runs
them -- `dbk_stage` (the clamped, field-aware staging with its dword and single-sample branches), `dbk_pass_x`, `dbk_pass_y` (with
`dbk_edge`, the rule itself) and `dbk_store` -- on a heap tile of the LDS tile's exact size, so an index outside the tile or outside a
frame is a sanitizer report.  What is not: the host form runs the 256 lanes of a phase one after the other where the GPU has a barrier,
so a missing barrier, a race between two lanes of one phase or anything the hardware does with LDS banks and unaligned dwords cannot
show here; those are covered by tests/test_gpu_deblock.py alone.

    python3 tools/check_deblock_host.py [--cxx /opt/rocm/llvm/bin/clang++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from savsr_amd.deblock import deblock_plane  # noqa: E402
from tests.deblock_cases import (BLOCKS, DEPTHS, LAST_SAMPLE, MODES, NO_EDGE, THRESHOLDS, as_bytes, case_frames, one_tile_plus,  # noqa: E402
                                 two_tiles_ragged)

HERE = os.path.join(ROOT, "tools", "host_check")


def build(cxx: str, work: str) -> str:
    src = open(os.path.join(ROOT, "savsr_amd", "csrc", "deblock.hip")).read()
    assert src.count('#include "common.hpp"') == 1
    with open(os.path.join(work, "deblock_device.inc"), "w") as f:
        f.write(src.replace('#include "common.hpp"', '#include "hip_stub.h"'))
    exe = os.path.join(work, "deblock_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", work, "-I", HERE,
                    "-I", os.path.join(ROOT, "savsr_amd", "csrc"), os.path.join(HERE, "deblock_main.cpp"), "-o", exe], check=True)
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "/opt/rocm/llvm/bin/clang++"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as work:
        exe = build(a.cxx, work)
        fin, fout = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")

        def call(args):
            return subprocess.run([exe] + [str(v) for v in args], capture_output=True, text=True)

        def run(m, depth=8, block=8, mode="weak", thr=(25, 13), interlaced=False, before=0, after=0, mis=0):
            n, r, c, step = m.shape
            raw = as_bytes(m)
            fb = before + raw.shape[1] + after
            frames = rng.integers(0, 256, (n, fb), dtype=np.uint8)
            frames[:, before:before + raw.shape[1]] = raw
            frames.tofile(fin)
            sh = depth - 8
            args = [8 if depth == 8 else 16, n, fb, before, r, c, step, depth, block, int(mode == "strong"), int(interlaced), thr[0] << sh, thr[1] << sh,
                    fb, before, mis, fin, fout]
            res = call(args)
            if res.returncode:
                raise SystemExit(f"FAILED {args}\n{res.stderr[-4000:]}")
            got = np.fromfile(fout, dtype=np.uint8).reshape(n, fb)
            want = np.empty_like(m)
            for t in range(n):
                for ch in range(step):
                    want[t, :, :, ch] = deblock_plane(m[t, :, :, ch], depth, block, mode, thr, interlaced)
            if not np.array_equal(got[:, before:before + raw.shape[1]], as_bytes(want)):
                raise SystemExit(f"MISMATCH {args}: {np.argwhere(got[:, before:before + raw.shape[1]] != as_bytes(want))[:5].tolist()}")
            if not (np.all(got[:, :before] == 0xA5) and np.all(got[:, before + raw.shape[1]:] == 0xA5)):
                raise SystemExit(f"WROTE OUTSIDE THE PLANE {args}")

        count = 0
        for block in BLOCKS:
            for mode in MODES:
                for interlaced in (False, True):
                    for r, c in NO_EDGE + (LAST_SAMPLE, (2, 9), (3, 17), (35, 21)):
                        run(case_frames(rng, 1, r, c, block=block), 8, block, mode, (25, 13), interlaced)
                        count += 1
                    run(case_frames(rng, 1, *one_tile_plus(1), block=block), 8, block, mode, (25, 13), interlaced)
                    run(case_frames(rng, 1, 37, 41, depth=10, above=True, block=block), 10, block, mode, (25, 13), interlaced, mis=2)
                    count += 2
        for mode in MODES:
            for interlaced in (False, True):
                run(case_frames(rng, 1, *two_tiles_ragged(1)), 8, 8, mode, (25, 13), interlaced)
                count += 1
        for depth in DEPTHS:
            for thr in THRESHOLDS:
                run(case_frames(rng, 1, 35, 45, depth=depth, above=True, noise=thr[0] == 255), depth, 8, "strong", thr, depth == 10)
                count += 1
        for step in (1, 2, 3, 4):          # steps, frames, planes inside frames at misaligned bases
            for n in (1, 3):
                for depth, before, after, mis in ((8, 0, 0, 0), (8, 5, 3, 1), (12, 6, 2, 2)):
                    run(case_frames(rng, n, 35, tile_plus(step), step=step, depth=depth, above=True), depth, 8, "strong", (25, 13), step == 3, before, after,
                        mis)
                    count += 1
        # the refusals: exit code 5, the entry named, nothing written
        np.zeros(64, np.uint8).tofile(fin)
        ok = [8, 1, 64, 0, 8, 8, 1, 8, 8, 0, 0, 25, 13, 64, 0, 0, fin, fout]
        for slot, bad, words in ((1, 0, "n_frames >= 1"), (4, 0, "rows >= 1"), (5, 0, "at least one sample"), (6, 5, "step 1 .. 4"), (8, 5, "block 4, 8 or 16"),
                                 (9, 2, "strong and interlaced 0 or 1"), (11, 256, "thresholds 0 .. 255"), (12, -1, "thresholds 0 .. 255"),
                                 (2, 63, "frame_bytes smaller"), (3, -1, "plane offsets >= 0"), (13, 63, "out_frame_bytes smaller")):
            args = list(ok)
            args[slot] = bad
            if slot == 2:
                args[13] = 64
            res = call(args)
            if res.returncode != 5 or "video_deblock_u8" not in res.stderr or words not in res.stderr:
                raise SystemExit(f"REFUSAL {args}: exit {res.returncode}, {res.stderr[-400:]!r} (expected {words!r})")
            count += 1
        np.zeros(128, np.uint8).tofile(fin)
        for args, words in (([16, 1, 128, 0, 8, 8, 1, 9, 8, 0, 0, 25, 13, 128, 0, 0, fin, fout], "depth 10 or 12"),
                            ([16, 1, 128, 0, 8, 8, 1, 10, 8, 0, 0, 25, 13, 128, 0, 1, fin, fout], "2-byte aligned"),
                            ([16, 1, 128, 0, 8, 8, 1, 10, 8, 0, 0, 1021, 13, 128, 0, 0, fin, fout], "thresholds 0 .. 255")):
            res = call(args)
            if res.returncode != 5 or "video_deblock_u16" not in res.stderr or words not in res.stderr:
                raise SystemExit(f"REFUSAL {args}: exit {res.returncode}, {res.stderr[-400:]!r} (expected {words!r})")
            count += 1
    print(f"ok: {count} cases equal the specification or are refused by name, no sanitizer report")


def tile_plus(step: int) -> int:
    """Columns of one tile plus a ragged rest at this step."""
    from tests.deblock_cases import tile_cols
    return tile_cols(step) + 5


if __name__ == "__main__":
    main()
