"""Golden fixtures of the I420 conversions (savsr_amd/yuv.py, yuv.hip): the REFERENCE's ycbcr2rgb / rgb2ycbcr on seeded inputs.

Build-container only (needs the reference checkout, see tools/ref_import.py): lbasicsr/utils/color_util.py is loaded by file path at
generation time; nothing of it is stored in the repository, the fixture holds inputs and recorded results.  Writes
tests/golden/yuv_outputs.npz:

  in/<h>x<w>/i420   uint8 [N, i420_bytes]      seeded random frames; "in/table" = one frame with all 256 Y values against a 16-step (U, V) grid
  in/<h>x<w>/rgb    float32 [N, 3, h, w]       np.clip(ycbcr2rgb(float32 samples / 255), 0, 1) after nearest chroma replication
  out/<h>x<w>/rgb   float32 [N, 3, h, w]       seeded, in [-0.1, 1.1]
  out/<h>x<w>/y, cb, cr   float64              rgb2ycbcr of the clamped input x 255 before rounding; box mean of the in-image pixels for chroma

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_yuv.py
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_import  # noqa: E402
from savsr_amd.yuv import BT601, chroma_hw, i420_bytes, split_planes  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SIZES = [(2, 2), (3, 5), (8, 10), (9, 14), (17, 33)]
FRAMES = 3
TIE_EPS = 1e-4              # a sample is near a tie when its float64 value lies within this of some k + 0.5 (tests/test_yuv.py)
TIE_SHARE = 1e-3            # at most this share of the output-side samples may be near a tie


def reference_color_util():
    sys.dont_write_bytecode = True
    path = os.path.join(ref_import.REF_ROOT, "lbasicsr", "utils", "color_util.py")
    spec = importlib.util.spec_from_file_location("ref_color_util", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def table_frame():
    """256 x 256 in 16 x 16 regions of 16 x 16 pixels: (U, V) = a 16-step grid (8, 24 .. 248) over the regions, Y = all 256 values in each."""
    h = w = 256
    i = np.arange(256)
    y = ((i[:, None] % 16) * 16 + i[None, :] % 16).astype(np.uint8)
    g = (np.arange(16) * 16 + 8).astype(np.uint8)
    u = np.repeat(np.repeat(g[:, None], 8, 0), 128, 1)                     # U steps every 8 chroma rows
    v = np.repeat(np.repeat(g[None, :], 8, 1), 128, 0)                     # V steps every 8 chroma columns
    return h, w, np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)])[None]


def input_side(cu, frames, h, w):
    y, u, v = split_planes(frames, h, w)
    u = np.repeat(np.repeat(u, 2, 1), 2, 2)[:, :h, :w]
    v = np.repeat(np.repeat(v, 2, 1), 2, 2)[:, :h, :w]
    ycc = np.stack([y, u, v], -1).astype(np.float32) / np.float32(255.0)             # [N, h, w, 3] float32 in [0, 1]
    rgb = np.clip(cu.ycbcr2rgb(ycc), 0, 1).astype(np.float32)
    return np.ascontiguousarray(rgb.transpose(0, 3, 1, 2))


def output_side(cu, x):
    n, _, H, W = x.shape
    p = np.clip(x, 0, 1).astype(np.float32).transpose(0, 2, 3, 1)
    # float32 in -> the reference computes in float64 (its matrix is a Python list) and returns float32 / 255: redo its last step in float64
    t = BT601["to_ycbcr"]
    ycc = np.matmul(p.astype(np.float64), np.array([t["y"], t["cb"], t["cr"]]).T) + np.array(t["offset"])
    ref = cu.rgb2ycbcr(p).astype(np.float64) * 255.0
    assert np.abs(ycc - ref).max() < 3e-5, np.abs(ycc - ref).max()          # (its float32 result: half an ulp at 1 x 255 = 1.5e-5)
    ch, cw = chroma_hw(H, W)
    pad = np.full((n, 2 * ch, 2 * cw, 3), np.nan)
    pad[:, :H, :W] = ycc
    box = np.nanmean(pad.reshape(n, ch, 2, cw, 2, 3), axis=(2, 4))
    return ycc[..., 0], box[..., 1], box[..., 2]


def near_tie(v):
    return np.abs(v - np.floor(v) - 0.5) <= TIE_EPS


def main():
    cu = reference_color_util()
    seed = 0
    while True:
        rng = np.random.RandomState(seed)
        out = {}
        th, tw, tf = table_frame()
        out["in/table/i420"] = tf
        out["in/table/rgb"] = input_side(cu, tf, th, tw)
        ties = total = 0
        for h, w in SIZES:
            fr = rng.randint(0, 256, size=(FRAMES, i420_bytes(h, w)), dtype=np.uint8)
            out[f"in/{h}x{w}/i420"] = fr
            out[f"in/{h}x{w}/rgb"] = input_side(cu, fr, h, w)
            x = rng.uniform(-0.1, 1.1, size=(FRAMES, 3, h, w)).astype(np.float32)
            y, cb, cr = output_side(cu, x)
            out[f"out/{h}x{w}/rgb"] = x
            out[f"out/{h}x{w}/y"], out[f"out/{h}x{w}/cb"], out[f"out/{h}x{w}/cr"] = y, cb, cr
            for v in (y, cb, cr):
                ties += int(near_tie(v).sum())
                total += v.size
        print(f"seed {seed}: {ties} of {total} output samples near a tie")
        if ties <= TIE_SHARE * total:
            break
        seed += 1
    out["seed"] = np.array(seed)
    np.savez_compressed(os.path.join(GOLD, "yuv_outputs.npz"), **out)
    print("wrote", os.path.getsize(os.path.join(GOLD, "yuv_outputs.npz")) / 1e3, "KB")


if __name__ == "__main__":
    main()
