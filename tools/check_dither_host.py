"""Host-side check of csrc/dither.hpp: the header the three quantiser files share, compiled unchanged into a stand-alone host program
(tools/host_check/dither_main.cpp) under -fsanitize=address,undefined and compared with the numpy specification (savsr_amd/dither.py):
theta at all 256 positions; the rule floor(t + theta) at all 256 positions over a sweep of t -- every j / 256 fraction at the codes of
tests/dither_cases.py, the ends of every range at each depth and their float32 neighbours; the clamped quantiser of the packed and luma
paths on values outside [0, 1], NaN and inf; the row / column split of a linear index on both sides of 2^32.  CPU only: nothing here is
loaded into Python or run on a GPU.

    python3 tools/check_dither_host.py [--cxx /opt/rocm/llvm/bin/clang++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from savsr_amd import dither as D  # noqa: E402
from savsr_amd import yuv  # noqa: E402
from tests import dither_cases as DC  # noqa: E402

HERE = os.path.join(ROOT, "tools", "host_check")


def build(cxx: str, work: str) -> str:
    exe = os.path.join(work, "dither_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "savsr_amd", "csrc"), os.path.join(HERE, "dither_main.cpp"), "-o", exe], check=True)
    return exe


def sweep() -> np.ndarray:
    """The values of t the rule is compared at, float32."""
    j = np.arange(256, dtype=np.float32) / np.float32(256)
    t = [np.float32(i) + j for i in DC.CONSTANT_I]
    ends = []
    for k in (1, 4, 16):
        ends += [0, 16 * k, 235 * k, 240 * k, 255 * k, 256 * k - 1]
    ends = np.array(sorted(set(ends)), np.float32)
    t += [ends, np.nextafter(ends, np.float32(-1)), np.nextafter(ends, np.float32(1e9)), ends + np.float32(0.5)]
    t.append(np.random.RandomState(0).uniform(0, 4096, size=4096).astype(np.float32))
    return np.concatenate(t).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "/opt/rocm/llvm/bin/clang++"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as work:
        exe = build(a.cxx, work)
        fin, fout = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")

        def run(op, data=None, n=0, mul=None, dtype=np.float32):
            args = [exe, str(op), fout]
            if data is not None:
                data.tofile(fin)
                args += [fin, str(n)] + ([] if mul is None else [repr(float(mul))])
            res = subprocess.run(args, capture_output=True, text=True)
            if res.returncode:
                raise SystemExit(f"FAILED op {op} (rc {res.returncode})\n{res.stderr[-4000:]}")
            return np.fromfile(fout, dtype=dtype)

        th = run(0).reshape(16, 16)
        if not np.array_equal(th, D.thresholds()):
            raise SystemExit("MISMATCH theta")
        t = sweep()
        got = run(1, t, t.size).reshape(t.size, 16, 16)
        want = D.dither_floor(np.ascontiguousarray(np.broadcast_to(t[:, None, None], (t.size, 16, 16))))
        if not np.array_equal(got, want):
            raise SystemExit(f"MISMATCH rule at t = {t[np.nonzero((got != want).any(axis=(1, 2)))[0][:8]]}")
        rng = np.random.RandomState(1)
        v = np.concatenate([rng.uniform(-0.2, 1.2, size=4096), [np.nan, np.inf, -np.inf, 0.0, 1.0, -0.0]]).astype(np.float32)
        for depth in DC.DEPTHS:
            got = run(2, v, v.size, 255 << (depth - 8), np.uint32).reshape(v.size, 16, 16)
            want = yuv.unit_to_luma(np.ascontiguousarray(np.broadcast_to(v[:, None, None], (v.size, 16, 16))), depth, dither="ordered")
            if not np.array_equal(got, want.astype(np.uint32)):
                raise SystemExit(f"MISMATCH quantiser at depth {depth}")
        rng = np.random.RandomState(2)
        widths = [1, 2, 3, 4, 5, 7, 16, 255, 256, 257, 1280, 1920, 4095, 4096, 7680, 65535, 65537, (1 << 30) + 1, (1 << 31) - 1]
        pw = [(p, w) for w in widths for p in (0, 1, w - 1, w, 17 * w + 5, (1 << 32) - w, (1 << 32) - 1, 1 << 32, (1 << 33) + 12345) if 0 <= p // w < (1 << 32)]
        pw += [(int(p), int(w)) for w in rng.randint(1, 1 << 13, size=200) for p in rng.randint(0, 1 << 32, size=20, dtype=np.int64)]
        pw = np.array(pw, np.int64)
        got = run(3, pw.reshape(-1), len(pw), dtype=np.uint32).reshape(-1, 2)
        if not np.array_equal(got.astype(np.int64), np.stack([pw[:, 0] // pw[:, 1], pw[:, 0] % pw[:, 1]], 1)):
            raise SystemExit("MISMATCH row / column")
    print(f"ok: theta at 256 positions, the rule at {t.size} values x 256 positions, the quantiser at {v.size} values x 3 depths and "
          f"{len(pw)} index splits equal the specification, no sanitizer report")


if __name__ == "__main__":
    main()
