"""Host-side memory check of csrc/dering.hip: its entries and device functions, compiled unchanged into a stand-alone host program
(tools/host_check/) under -fsanitize=address,undefined, run one thread at a time on exact-size heap buffers and compared with the numpy
specification (savsr_amd/dering.py `dering_matrix` / `dering_fields`) on the shapes of tests/dering_cases.py: planes of 1 x 1, 1 x 9,
9 x 1, 7 x 7, 8 x 8 and 9 x 9, one tile plus a row and a column, two tiles each way with a ragged rest, progressive and field-wise with
1, 2 and 17 rows, every depth with samples above it, the strengths (0, 0), (0, 2), (4, 0), (15, 4) and the defaults on the case picture,
on noise and on constant blocks, dampings 3 and 6, steps 1 .. 4, 1 and 3 frames, planes inside frames at misaligned bases, and the
entries' refusals.  CPU only: nothing here is loaded into Python or run on a GPU.

What is covered: the two entries with their refusals and the job they build, and the three phases of the tiled kernel as the GPU runs
them -- `drg_stage` (the clamped, field-aware staging with its dword and single-sample branches), `drg_blocks` (with `drg_direction` and
`drg_primary8`, steps 1 and 2 of the rule) and `drg_filter` (with `drg_sample`, step 3, and the dword and single-sample stores) -- on heap
buffers of the LDS arrays' exact sizes, so an index outside the tile, the block words or a frame is a sanitizer report, and a signed
overflow in the costs is one too.  What is not: the host form runs the 256 lanes of a phase one after the other where the GPU has a
barrier, so a missing barrier or anything the hardware does with LDS banks and unaligned dwords cannot show here; those are covered by
tests/test_gpu_dering.py alone.

    python3 tools/check_dering_host.py [--cxx /opt/rocm/llvm/bin/clang++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from savsr_amd.dering import dering_plane  # noqa: E402
from tests.dering_cases import (DAMPINGS, DEPTHS, FIELD_ROWS, SMALL, STRENGTHS, as_bytes, case_frames, one_tile_plus, tile_cols,  # noqa: E402
                                two_tiles_ragged)

HERE = os.path.join(ROOT, "tools", "host_check")


def build(cxx: str, work: str) -> str:
    src = open(os.path.join(ROOT, "savsr_amd", "csrc", "dering.hip")).read()
    assert src.count('#include "common.hpp"') == 1
    with open(os.path.join(work, "dering_device.inc"), "w") as f:
        f.write(src.replace('#include "common.hpp"', '#include "hip_stub.h"'))
    exe = os.path.join(work, "dering_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", work, "-I", HERE,
                    "-I", os.path.join(ROOT, "savsr_amd", "csrc"), os.path.join(HERE, "dering_main.cpp"), "-o", exe], check=True)
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

        def run(m, depth=8, strength=(4, 2), damping=5, interlaced=False, before=0, after=0, mis=0):
            n, r, c, step = m.shape
            raw = as_bytes(m)
            fb = before + raw.shape[1] + after
            frames = rng.integers(0, 256, (n, fb), dtype=np.uint8)
            frames[:, before:before + raw.shape[1]] = raw
            frames.tofile(fin)
            sh = depth - 8
            args = [8 if depth == 8 else 16, n, fb, before, r, c, step, depth, int(interlaced), strength[0] << sh, strength[1] << sh, damping,
                    fb, before, mis, fin, fout]
            res = call(args)
            if res.returncode:
                raise SystemExit(f"FAILED {args}\n{res.stderr[-4000:]}")
            got = np.fromfile(fout, dtype=np.uint8).reshape(n, fb)
            want = np.empty_like(m)
            for t in range(n):
                for ch in range(step):
                    want[t, :, :, ch] = dering_plane(m[t, :, :, ch], depth, strength, damping, interlaced)
            if not np.array_equal(got[:, before:before + raw.shape[1]], as_bytes(want)):
                raise SystemExit(f"MISMATCH {args}: {np.argwhere(got[:, before:before + raw.shape[1]] != as_bytes(want))[:5].tolist()}")
            if not (np.all(got[:, :before] == 0xA5) and np.all(got[:, before + raw.shape[1]:] == 0xA5)):
                raise SystemExit(f"WROTE OUTSIDE THE PLANE {args}")

        count = 0
        for interlaced in (False, True):
            for r, c in SMALL + ((3, 17), (35, 21)) + (tuple((r, 21) for r in FIELD_ROWS) if interlaced else ()):
                run(case_frames(rng, 1, r, c, kind="noise" if r * c < 64 else "case"), interlaced=interlaced)
                count += 1
            run(case_frames(rng, 1, *one_tile_plus(1)), interlaced=interlaced)
            run(case_frames(rng, 1, *two_tiles_ragged(1)), interlaced=interlaced)
            run(case_frames(rng, 1, 37, 41, depth=10, above=True), 10, interlaced=interlaced, mis=2)
            count += 3
        for depth in DEPTHS:
            for strength in STRENGTHS:
                for kind in ("case", "noise", "blocks"):
                    run(case_frames(rng, 1, 35, 45, depth=depth, above=True, kind=kind), depth, strength, 5, depth == 10)
                    count += 1
            for damping in DAMPINGS:
                run(case_frames(rng, 1, 35, 45, depth=depth, above=True), depth, (15, 4), damping)
                run(case_frames(rng, 1, 19, 23, depth=depth, kind="noise"), depth, (7, 1), damping, True)
                count += 2
        for step in (1, 2, 3, 4):          # steps, frames, planes inside frames at misaligned bases
            for n in (1, 3):
                for depth, before, after, mis in ((8, 0, 0, 0), (8, 5, 3, 1), (12, 6, 2, 2)):
                    run(case_frames(rng, n, 35, tile_cols(step) + 5, step=step, depth=depth, above=True), depth, (4, 2), 5, step == 3, before, after, mis)
                    count += 1
        # the refusals: exit code 5, the entry named, nothing written
        np.zeros(64, np.uint8).tofile(fin)
        ok = [8, 1, 64, 0, 8, 8, 1, 8, 0, 4, 2, 5, 64, 0, 0, fin, fout]
        for slot, bad, words in ((1, 0, "n_frames >= 1"), (4, 0, "rows >= 1"), (5, 0, "at least one sample"), (6, 5, "step 1 .. 4"),
                                 (8, 2, "interlaced 0 or 1"), (9, 16, "pri a multiple"), (9, -1, "pri a multiple"), (10, 5, "sec a multiple"),
                                 (11, 2, "damping 3 .. 6"), (11, 7, "damping 3 .. 6"), (2, 63, "frame_bytes smaller"), (3, -1, "plane offsets >= 0"),
                                 (12, 63, "out_frame_bytes smaller")):
            args = list(ok)
            args[slot] = bad
            res = call(args)
            if res.returncode != 5 or "video_dering_u8" not in res.stderr or words not in res.stderr:
                raise SystemExit(f"REFUSAL {args}: exit {res.returncode}, {res.stderr[-400:]!r} (expected {words!r})")
            count += 1
        np.zeros(128, np.uint8).tofile(fin)
        for args, words in (([16, 1, 128, 0, 8, 8, 1, 9, 0, 16, 8, 5, 128, 0, 0, fin, fout], "depth 10 or 12"),
                            ([16, 1, 128, 0, 8, 8, 1, 8, 0, 4, 2, 5, 128, 0, 0, fin, fout], "depth 10 or 12 (8 bits: savsr_video_dering_u8)"),
                            ([16, 1, 128, 0, 8, 8, 1, 10, 0, 16, 8, 5, 128, 0, 1, fin, fout], "2-byte aligned"),
                            ([16, 1, 128, 0, 8, 8, 1, 10, 0, 18, 8, 5, 128, 0, 0, fin, fout], "pri a multiple"),
                            ([16, 1, 128, 0, 8, 8, 1, 10, 0, 16, 20, 5, 128, 0, 0, fin, fout], "sec a multiple")):
            res = call(args)
            if res.returncode != 5 or "video_dering_u16" not in res.stderr or words not in res.stderr:
                raise SystemExit(f"REFUSAL {args}: exit {res.returncode}, {res.stderr[-400:]!r} (expected {words!r})")
            count += 1
    print(f"ok: {count} cases equal the specification or are refused by name, no sanitizer report")


if __name__ == "__main__":
    main()
