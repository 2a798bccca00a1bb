"""Golden fixtures of the 4:2:2 / 4:4:4 conversions (savsr_amd/yuv.py with chroma=, yuv.hip): the REFERENCE's ycbcr2rgb / rgb2ycbcr on
seeded inputs, the recipe of tools/gen_golden_yuv.py with the layout's block in place of the 2 x 2 one.

Build-container only (needs the reference checkout, see tools/ref_import.py): lbasicsr/utils/color_util.py is loaded by file path at
generation time; nothing of it is stored in the repository, the fixture holds inputs and recorded results.  Writes
tests/golden/yuv_chroma_outputs.npz, for L in 422, 444:

  in/<L>/<h>x<w>/yuv   uint8 [N, frame_bytes]     seeded random frames of the layout
  in/<L>/<h>x<w>/rgb   float32 [N, 3, h, w]       np.clip(ycbcr2rgb(float32 samples / 255), 0, 1) after the layout's nearest replication
  out/<h>x<w>/rgb      float32 [N, 3, h, w]       seeded, in [-0.1, 1.1] (one input for both layouts)
  out/<L>/<h>x<w>/y, cb, cr   float64             rgb2ycbcr of the clamped input x 255 before rounding; chroma = the mean over the
                                                  layout's block (a pair, the pixel alone in the last column of an odd w; the pixel)

No 256 x 256 table frame: the per-sample tables are pinned by tests/golden/yuv_outputs.npz.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_yuv_chroma.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden_yuv import FRAMES, GOLD, SIZES, TIE_SHARE, near_tie, reference_color_util  # noqa: E402
from savsr_amd.yuv import BT601, chroma_hw, frame_bytes, replicate_chroma, split_planes  # noqa: E402

LAYOUTS = ("422", "444")


def input_side(cu, frames, h, w, chroma):
    y, u, v = split_planes(frames, h, w, 8, chroma)
    u, v = replicate_chroma(u, h, w, chroma), replicate_chroma(v, h, w, chroma)
    ycc = np.stack([y, u, v], -1).astype(np.float32) / np.float32(255.0)             # [N, h, w, 3] float32 in [0, 1]
    rgb = np.clip(cu.ycbcr2rgb(ycc), 0, 1).astype(np.float32)
    return np.ascontiguousarray(rgb.transpose(0, 3, 1, 2))


def output_side(cu, x, chroma):
    n, _, H, W = x.shape
    p = np.clip(x, 0, 1).astype(np.float32).transpose(0, 2, 3, 1)
    # float32 in -> the reference computes in float64 (its matrix is a Python list) and returns float32 / 255: redo its last step in float64
    t = BT601["to_ycbcr"]
    ycc = np.matmul(p.astype(np.float64), np.array([t["y"], t["cb"], t["cr"]]).T) + np.array(t["offset"])
    ref = cu.rgb2ycbcr(p).astype(np.float64) * 255.0
    assert np.abs(ycc - ref).max() < 3e-5, np.abs(ycc - ref).max()          # (its float32 result: half an ulp at 1 x 255 = 1.5e-5)
    ch, cw = chroma_hw(H, W, chroma)
    sx = W // cw + (W % cw > 0)                                              # 2 (4:2:2) or 1 (4:4:4); rows are never shared
    pad = np.full((n, H, sx * cw, 3), np.nan)
    pad[:, :, :W] = ycc
    box = np.nanmean(pad.reshape(n, H, cw, sx, 3), axis=3)
    return ycc[..., 0], box[..., 1], box[..., 2]


def main():
    cu = reference_color_util()
    seed = 0
    while True:
        rng = np.random.RandomState(seed)
        out = {}
        ties = total = 0
        for h, w in SIZES:
            for lay in LAYOUTS:
                fr = rng.randint(0, 256, size=(FRAMES, frame_bytes(h, w, 8, lay)), dtype=np.uint8)
                out[f"in/{lay}/{h}x{w}/yuv"] = fr
                out[f"in/{lay}/{h}x{w}/rgb"] = input_side(cu, fr, h, w, lay)
            x = rng.uniform(-0.1, 1.1, size=(FRAMES, 3, h, w)).astype(np.float32)
            out[f"out/{h}x{w}/rgb"] = x
            for lay in LAYOUTS:
                y, cb, cr = output_side(cu, x, lay)
                out[f"out/{lay}/{h}x{w}/y"], out[f"out/{lay}/{h}x{w}/cb"], out[f"out/{lay}/{h}x{w}/cr"] = y, cb, cr
                for v in (y, cb, cr):
                    ties += int(near_tie(v).sum())
                    total += v.size
        print(f"seed {seed}: {ties} of {total} output samples near a tie")
        if ties <= TIE_SHARE * total:
            break
        seed += 1
    out["seed"] = np.array(seed)
    path = os.path.join(GOLD, "yuv_chroma_outputs.npz")
    np.savez_compressed(path, **out)
    print("wrote", os.path.getsize(path) / 1e3, "KB")


if __name__ == "__main__":
    main()
