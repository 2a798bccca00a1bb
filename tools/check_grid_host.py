"""Host-side memory check of csrc/grid.hip and of the origin path of csrc/deblock.hip: their entries and device functions, compiled
unchanged into a stand-alone host program (tools/host_check/grid_main.cpp) under -fsanitize=address,undefined, run one thread at a time
on exact-size heap buffers and compared with the numpy specifications (savsr_amd/grid.py `grid_stats_matrix`, savsr_amd/deblock.py
`deblock_plane` with an origin) on the shapes of tests/grid_cases.py and tests/deblock_cases.py.  CPU only: nothing here is loaded into
Python or run on a GPU.

What is covered.  grid.hip: the two entries with their refusals and the job they build; `gs_load` in both forms (the 16-byte piece with
the dwords of its neighbours, the single samples), `gs_band` (the four-row window, the packed counters, the cells) at steps 1 .. 4,
depths 8 / 10 / 12 with samples above the top, progressive and field-wise with odd row counts, planes below one boundary, one band and
one workgroup plus ragged rests, misaligned planes inside frames, several frames, two calls adding into one table.  deblock.hip: the
`_o` entries with every origin of block 8 and the corner origins of 4 and 16 on the cover plane, planes whose P side lies beyond them,
one tile plus a row and a column and two ragged tiles at steps 1, 3, 4 and depths 8 / 12, both modes, progressive and field-wise -- the
tile origins are negative there, so an index outside the staged tile or outside a frame is a sanitizer report.  What is not: the host
form runs the lanes one after the other and every lane adds its own counts, so the LDS cells, their atomics and the barriers around
them cannot show here; tests/test_gpu_grid.py covers those.

    python3 tools/check_grid_host.py [--cxx /opt/rocm/llvm/bin/clang++]
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
from savsr_amd.grid import grid_stats_matrix  # noqa: E402
from tests.deblock_cases import COVER_SHAPE, as_bytes, case_frames, one_tile_plus, two_tiles_ragged  # noqa: E402
from tests.grid_cases import stats_frames, stats_tile  # noqa: E402

HERE = os.path.join(ROOT, "tools", "host_check")


def build(cxx: str, work: str) -> str:
    for name in ("deblock", "grid"):
        src = open(os.path.join(ROOT, "savsr_amd", "csrc", f"{name}.hip")).read()
        assert src.count('#include "common.hpp"') == 1
        with open(os.path.join(work, f"{name}_device.inc"), "w") as f:
            f.write(src.replace('#include "common.hpp"', '#include "hip_stub.h"'))
    exe = os.path.join(work, "grid_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", work, "-I", HERE,
                    "-I", os.path.join(ROOT, "savsr_amd", "csrc"), os.path.join(HERE, "grid_main.cpp"), "-o", exe], check=True)
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

        def frames_of(m, before, after):
            raw = as_bytes(m)
            fb = before + raw.shape[1] + after
            frames = rng.integers(0, 256, (m.shape[0], fb), dtype=np.uint8)
            frames[:, before:before + raw.shape[1]] = raw
            frames.tofile(fin)
            return raw, fb

        def stats(m, depth=8, interlaced=False, cap=32, before=0, after=0, mis=0, calls=1):
            n, r, c, step = m.shape
            _, fb = frames_of(m, before, after)
            args = ["stats", 8 if depth == 8 else 16, n, fb, before, r, c, step, depth, int(interlaced), cap, calls, mis, 0, fin, fout]
            res = call(args)
            if res.returncode:
                raise SystemExit(f"FAILED {args}\n{res.stderr[-4000:]}")
            got = np.fromfile(fout, dtype=np.int64).reshape(n, 2, 16)
            want = np.stack([sum(grid_stats_matrix(m[t, :, :, ch], depth, interlaced, cap) for ch in range(step)) for t in range(n)]) * calls
            if not np.array_equal(got, want):
                raise SystemExit(f"MISMATCH {args}: {np.argwhere(got != want)[:5].tolist()}")

        def deblock(m, depth, block, mode, interlaced, origin, before=0, after=0, mis=0):
            n, r, c, step = m.shape
            raw, fb = frames_of(m, before, after)
            sh = depth - 8
            args = ["deblock", 8 if depth == 8 else 16, n, fb, before, r, c, step, depth, block, int(mode == "strong"), int(interlaced), 25 << sh, 13 << sh,
                    origin[0], origin[1], mis, fin, fout]
            res = call(args)
            if res.returncode:
                raise SystemExit(f"FAILED {args}\n{res.stderr[-4000:]}")
            got = np.fromfile(fout, dtype=np.uint8).reshape(n, fb)
            want = np.empty_like(m)
            for t in range(n):
                for ch in range(step):
                    want[t, :, :, ch] = deblock_plane(m[t, :, :, ch], depth, block, mode, (25, 13), interlaced, origin)
            if not np.array_equal(got[:, before:before + raw.shape[1]], as_bytes(want)):
                raise SystemExit(f"MISMATCH {args}: {np.argwhere(got[:, before:before + raw.shape[1]] != as_bytes(want))[:5].tolist()}")
            if not (np.all(got[:, :before] == 0xA5) and np.all(got[:, before + raw.shape[1]:] == 0xA5)):
                raise SystemExit(f"WROTE OUTSIDE THE PLANE {args}")

        count = 0
        # ---- the statistics
        for r, c in ((1, 1), (3, 3), (4, 4), (2, 9), (9, 2), (5, 37), (8, 64), (17, 48), (35, 33)):
            for interlaced in (False, True):
                stats(stats_frames(rng, 1, r, c), 8, interlaced)
                count += 1
        tr, tc = stats_tile()
        for r, c in ((tr + 1, 64), (2 * tr + 5, 80), (tr, tc + 16), (tr + 3, 2 * tc + 48)):          # one band / one workgroup plus ragged rests
            stats(stats_frames(rng, 1, r, c), 8, r % 2 == 1)
            count += 1
        for step in (1, 2, 3, 4):
            for depth, before, after, mis in ((8, 0, 0, 0), (8, 5, 3, 1), (10, 6, 2, 2), (12, 16, 0, 0)):
                cols = 16 * (5 if step != 3 else 3) if (before % 16 == 0 and mis == 0) else 37
                stats(stats_frames(rng, 3 if step == 1 else 1, 21, cols, step=step, depth=depth, above=True), depth, step == 3, 32, before, after, mis)
                count += 1
        for cap in (0, 1, 255):
            stats(stats_frames(rng, 1, 19, 48), 8, False, cap)
            count += 1
        stats(stats_frames(rng, 3, 18, 32), 8, True, 32, calls=2)          # frames do not leak into each other; calls add
        stats(stats_frames(rng, 2, 7, 23, depth=12, above=True), 12, True, 32, 4, 2, 2, calls=2)
        count += 2
        # ---- the deblocker with an origin
        for block, origins in ((8, [(y, x) for y in range(8) for x in range(8)]), (4, [(1, 1), (3, 3)]), (16, [(1, 1), (15, 15)])):
            for o in origins:
                deblock(case_frames(rng, 1, *COVER_SHAPE, block=block), 8, block, "strong", False, o)
                count += 1
                if o[0] % 2 == 0:
                    deblock(case_frames(rng, 1, *COVER_SHAPE, block=block), 8, block, "weak", True, o)
                    count += 1
        for r, c in ((1, 1), (2, 9), (9, 2)):
            deblock(case_frames(rng, 1, r, c), 8, 8, "strong", False, (1, 1))
            count += 1
        for step in (1, 3, 4):
            for shape in (one_tile_plus(step), two_tiles_ragged(step)):
                for o, depth, mode, interlaced in (((1, 1), 8, "weak", False), ((7, 5), 12, "strong", False), ((6, 5), 8, "strong", True),
                                                   ((2, 1), 12, "weak", True)):
                    mis = 2 if depth == 12 else 1
                    deblock(case_frames(rng, 1, *shape, step=step, depth=depth, above=True), depth, 8, mode, interlaced, o, 6 if mis else 0, 2, mis)
                    count += 1
        # ---- the refusals: exit code 5, the entry named
        np.zeros(256, np.uint8).tofile(fin)
        ok = ["stats", 8, 1, 64, 0, 8, 8, 1, 8, 0, 32, 1, 0, 0, fin, fout]
        for slot, bad, words in ((2, 0, "n_frames >= 1"), (5, 0, "rows >= 1"), (6, 0, "at least one sample"), (7, 5, "step 1 .. 4"), (7, 0, "step 1 .. 4"),
                                 (3, 63, "frame_bytes smaller"), (4, -1, "plane offsets >= 0"), (13, 4, "8-byte aligned"), (10, -1, "cap 0 .. 255"),
                                 (10, 256, "cap 0 .. 255"), (9, 2, "interlaced 0 or 1")):
            args = list(ok)
            args[slot] = bad
            res = call(args)
            if res.returncode != 5 or "video_grid_stats_u8" not in res.stderr or words not in res.stderr:
                raise SystemExit(f"REFUSAL {args}: exit {res.returncode}, {res.stderr[-400:]!r} (expected {words!r})")
            count += 1
        for args, words in ((["stats", 16, 1, 128, 0, 8, 8, 1, 9, 0, 32, 1, 0, 0, fin, fout], "depth 10 or 12"),
                            (["stats", 16, 1, 128, 0, 8, 8, 1, 10, 0, 32, 1, 1, 0, fin, fout], "2-byte aligned"),
                            (["stats", 16, 1, 129, 0, 8, 8, 1, 10, 0, 32, 1, 0, 0, fin, fout], "2-byte aligned")):
            res = call(args)
            if res.returncode != 5 or "video_grid_stats_u16" not in res.stderr or words not in res.stderr:
                raise SystemExit(f"REFUSAL {args}: exit {res.returncode}, {res.stderr[-400:]!r} (expected {words!r})")
            count += 1
        okd = ["deblock", 8, 1, 64, 0, 8, 8, 1, 8, 8, 0, 0, 25, 13, 0, 0, 0, fin, fout]
        for changes, words in (({15: 8}, "origin_y and origin_x 0 .. block - 1"), ({14: -1}, "origin_y and origin_x 0 .. block - 1"),
                               ({9: 4, 15: 4}, "origin_y and origin_x 0 .. block - 1"), ({11: 1, 14: 3}, "origin_y even with interlaced")):
            args = list(okd)
            for k, v in changes.items():
                args[k] = v
            res = call(args)
            if res.returncode != 5 or "video_deblock_u8_o" not in res.stderr or words not in res.stderr:
                raise SystemExit(f"REFUSAL {args}: exit {res.returncode}, {res.stderr[-400:]!r} (expected {words!r})")
            count += 1
    print(f"ok: {count} cases equal the specification or are refused by name, no sanitizer report")


if __name__ == "__main__":
    main()
