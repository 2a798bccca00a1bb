"""Host-side memory check of csrc/surface.hip: its device functions, compiled unchanged into a stand-alone host program
(tools/host_check/) under -fsanitize=address,undefined, run one thread at a time over the tests' cases (tests/surface_cases.py) on
exact-size heap buffers and are compared with the numpy specification (savsr_amd/surface.py).  CPU only: nothing here is loaded into
Python or run on a GPU.  The host build takes the plain-C++ branch of `perm` (v_perm_b32 exists on the device only); everything else is
the code the GPU runs.  A surface block ends with the last byte that holds a sample, so a read of row padding behind the last row, or a
write behind a frame's resolved bytes, is a sanitizer report.

    python3 tools/check_surface_host.py [--cxx /opt/rocm/llvm/bin/clang++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from savsr_amd import surface as S  # noqa: E402
from tests import surface_cases as SC  # noqa: E402

HERE = os.path.join(ROOT, "tools", "host_check")


def build(cxx: str, work: str) -> str:
    src = open(os.path.join(ROOT, "savsr_amd", "csrc", "surface.hip")).read()
    assert src.count('#include "common.hpp"') == 1
    with open(os.path.join(work, "surface_device.inc"), "w") as f:
        f.write(src.replace('#include "common.hpp"', ""))
    exe = os.path.join(work, "surface_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", work, "-I", HERE,
                    "-I", os.path.join(ROOT, "savsr_amd", "csrc"), os.path.join(HERE, "surface_main.cpp"), "-o", exe], check=True)
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "/opt/rocm/llvm/bin/clang++"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as work:
        exe = build(a.cxx, work)
        fin, fdesc, fout = (os.path.join(work, f) for f in ("in.bin", "desc.bin", "out.bin"))

        def run(op, case, frames, n, stride, mis):
            tab = case.table
            S.descriptor(tab).tofile(fdesc)
            frames.tofile(fin)
            args = [op, n, stride, tab.bytes, tab.span, case.h, case.w, case.depth, S.LAYOUTS.index(case.layout), int(tab.msb), len(tab.planes), mis,
                    fin, fdesc, fout]
            res = subprocess.run([exe] + [str(v) for v in args], capture_output=True, text=True)
            if res.returncode:
                raise SystemExit(f"FAILED {case.id} {args}\n{res.stderr[-4000:]}")
            return np.fromfile(fout, dtype=np.uint8)

        count = 0
        for case in SC.CASES:
            tab = case.table
            surf, planar = SC.surface_frames(case), SC.planar_frames(case)
            n, stride = surf.shape
            two = tab.sample == 2
            for mis in (0, 2 if two else 1):
                # unpack: the block ends with the last sample of the last frame
                got = run(0, case, surf.reshape(-1)[:(n - 1) * stride + tab.span], n, stride, mis).reshape(n, -1)
                if not np.array_equal(got, S.unpack_frames(surf, case.surface, case.h, case.w, case.depth, case.layout)):
                    raise SystemExit(f"MISMATCH unpack {case.id} misalign {mis}")
                # pack: 0xA5 outside the frames' resolved bytes stays, every byte inside is the specification's
                got = run(1, case, planar, n, stride, mis)
                want = np.full((n, stride), 0xA5, dtype=np.uint8)
                want[:, :tab.bytes] = S.pack_frames(planar, case.surface, case.h, case.w, case.depth, case.layout)
                if not np.array_equal(got, want.reshape(-1)[:got.size]) or got.size != (n - 1) * stride + tab.bytes:
                    raise SystemExit(f"MISMATCH pack {case.id} misalign {mis}")
                count += 2
    print(f"ok: {count} cases equal the specification, no sanitizer report")


if __name__ == "__main__":
    main()
