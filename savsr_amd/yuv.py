"""Planar YUV 4:2:0 (I420) <-> RGB, the host restatement that specifies savsr_video_gather_i420 / savsr_video_quantize_i420 (yuv.hip);
with `chroma=` also 4:2:2 and 4:4:4 (savsr_video_gather_yuvp / savsr_video_quantize_yuvp, see "Chroma layouts" below) and with `siting=`
the chroma siting and a linear chroma reconstruction (savsr_video_gather_yuvs / savsr_video_quantize_yuvs, see "Chroma siting" below).

The default colour matrix is the reference's (lbasicsr/utils/color_util.py, `rgb2ycbcr` / `ycbcr2rgb`: ITU-R BT.601, limited range,
Matlab's rounded constants: `BT601`), the same whose Y row metrics.py uses for PSNR-Y.  4:2:0 only, at 8, 10 or 12 bits (`depth=`;
10 and 12 with the limited-range colour spaces only, see "High depth" below).  `COLOURS` names the four
colour spaces served (`colour=`; the position is the id of the C ABI) and `matrix(name)` gives each one's coefficient table: BT601
itself for "bt601", built from (Kr, Kb, range) for the others (`kYuv` is the twin in yuv.hip, the same float64 expressions).

I420 frame of an h x w picture: h * w Y bytes, then ch * cw U (Cb) bytes, then ch * cw V (Cr) bytes, ch = (h + 1) // 2,
cw = (w + 1) // 2 -- the frame as it lies in a Y4M file.  A video is a uint8 array [N, i420_bytes(h, w)].

Both directions are float32 with a fixed operation order and no fused multiply-add, so that numpy and the kernels agree bit for bit:

  i420_to_rgb   per-sample tables (a float64 product, plus the channel's offset where it is folded in, rounded once to float32: what
                a C++ constant expression gives), summed in float32 in a fixed order, clamped to [0, 1]; chroma replicated over its
                2 x 2 block.  Not rounded to 8 bits.
  rgb_to_i420   RGB clamped to [0, 1]; Y per pixel; Cb / Cr from the mean RGB of the block's in-image pixels (1, 2 or 4: the
                divisor is a power of two); every product and every sum rounded to float32; round half to even (tensor2img's rule);
                full range only: clipped to 0 .. 255 after the rounding (pure red has Cr = 255.5, pure blue Cb = 255.5 -> 256).

High depth (d = 10 or 12, k = 2^(d - 8); the specification of savsr_video_gather_yuv420_16 / savsr_video_quantize_yuv420_16).  A frame is
the 8-bit frame's planes with every sample a little-endian 16-bit word, as it lies in a Y4M file tagged C420p10 / C420p12: a video is a
uint8 array [N, 2 * i420_bytes(h, w)] (`i420_bytes(h, w, d)`), never a uint16 one.  Limited range only: a sample is the 8-bit one times k
(Y = 16 k .. 235 k), so every constant is the 8-bit table's, scaled by a power of two; full range at depth d scales by 2^d - 1 instead
and has no definition here.

  i420_to_rgb   no tables: with c = float32(coef / k) and o = float32(offset / 255), Yt = s_y * c_y, R = (Yt + s_v * c_rv) + o_R,
                G = ((Yt + s_u * c_gu) + s_v * c_gv) + o_G, B = (Yt + s_u * c_bu) + o_B in float32, every product and sum rounded;
                clamped to [0, 1].  A sample above 2^d - 1 is read as 2^d - 1.  At most five roundings of values below 2.5, so the result
                lies within 5 * 2.5 * 2^-24 < 1e-6 of the float64 closed form.
  rgb_to_i420   rint(ycbcr_f32 * k), half to even (the product by k is exact); Y in 16 k .. 235 k and chroma in 16 k .. 240 k, no clip.

Chroma layouts (`chroma=` "420", "422" or "444"; the position in CHROMAS is the id of the C ABI, SAVSR_CHROMA_*).  A frame holds h * w Y
samples, then ch * cw U samples, then ch * cw V samples with (ch, cw) = `chroma_hw(h, w, chroma)`: (ceil(h / 2), ceil(w / 2)) for 4:2:0,
(h, ceil(w / 2)) for 4:2:2 and (h, w) for 4:4:4; `frame_bytes(h, w, depth, chroma)` bytes, the samples as wide as above.  The arithmetic
is 4:2:0's with another block shape and nothing else: to RGB, chroma sample (cy, cx) serves pixels (cy, 2 cx .. 2 cx + 1) in 4:2:2 and
pixel (cy, cx) in 4:4:4 (nearest replication); from RGB, Cb / Cr come from the mean RGB of the block's in-image pixels, (a + b) * 0.5
for a 4:2:2 pair, the pixel alone in the last column of an odd W, and the pixel's own clamped RGB in 4:4:4 (no mean).  That pair --
nearest up, box down -- is what `siting=None` runs; it models no chroma siting.

Chroma siting (`siting=` None or one of SITINGS; the position in SITINGS plus one is the id of the C ABI, SAVSR_SITING_*, 0 = None;
the specification of savsr_video_gather_yuvs / savsr_video_quantize_yuvs).  Where chroma sample (cy, cx) lies, in luma pixel coordinates:

    siting      4:2:0 x      4:2:0 y      4:2:2 x      4:2:2 y
    centre      2 cx + 0.5   2 cy + 0.5   2 cx + 0.5   cy           JPEG, MPEG-1 (Y4M's C420jpeg)
    left        2 cx         2 cy + 0.5   2 cx         cy           MPEG-2, H.264, HEVC 4:2:0 and every standard 4:2:2 (C420mpeg2)
    topleft     2 cx         2 cy         refused      refused      (C420paldv, as ffmpeg maps it); 4:2:2 has no vertical subsampling

4:4:4 has nothing to resample: any siting there runs the code of siting=None and gives its bytes.

  i420_to_rgb   chroma at every luma pixel is the separable linear interpolation between the two nearest chroma samples at the positions
                above, edge samples replicated, samples above 2^d - 1 clipped first (`interpolate_chroma`).  Per subsampled axis, for
                pixel 2 c and pixel 2 c + 1:  centre (3 C[c] + C[c - 1]) / 4 and (3 C[c] + C[c + 1]) / 4;  cosited C[c] and
                (C[c] + C[c + 1]) / 2.  The value is an integer numerator (at most 4095 * 16) times 2^-4 (4:2:0) or 2^-2 (4:2:2): exact
                in float32 whatever the order.  It then takes the coefficient arithmetic of "High depth" at every depth, 8 included
                (k = 1, so all four colour spaces at 8 bits; limited range only at 10 / 12 as ever): the same bound, within
                5 * 2.5 * 2^-24 < 1e-6 of the float64 closed form.  Constant chroma planes therefore give the RGB of siting=None bit for
                bit at 10 / 12 bits and within 1e-6 at 8 bits (the table path and the coefficient path round differently).
  rgb_to_i420   None and "centre" are `_block_mean`, bit for bit: the box is the centre-sited filter.  Cosited axes take [1 2 1] / 4:
                h3(l, c, r) = ((l + r) + (c + c)) * 0.25 in float32, every tap index clamped into the image (`filter_chroma_rgb`).
                left, 4:2:2: h3(p[y, 2 cx - 1], p[y, 2 cx], p[y, 2 cx + 1]) = Hrow(y).  left, 4:2:0: (Hrow(2 cy) + Hrow(2 cy + 1)) * 0.5,
                Hrow(2 cy) alone on the last row of an odd H.  topleft, 4:2:0: ((Hrow(2 cy - 1) + Hrow(2 cy + 1)) + (Hrow(2 cy) +
                Hrow(2 cy))) * 0.25, rows clamped.  `_row`, the product by k, rint and the full-range clip follow as without a siting.

Filters longer than linear, PAL-DV's alternating Cb / Cr lines (read as topleft, as ffmpeg does), the vertical chroma positions of
interlaced 4:2:0 (savsr_amd/deinterlace.py turns the fields into progressive frames first; the planes are then read as progressive ones) and
4:1:1 are not modelled.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from .dither import check_dither, dither_floor

# BT.601 limited range, the reference's constants.  to_rgb: ycbcr2rgb's matrix entries (per 8-bit step, result in [0, 1]) and its
# offsets (in 8-bit steps, / 255 -> [0, 1]).  to_ycbcr: rgb2ycbcr's rows (8-bit steps per unit of RGB in [0, 1]) and offsets.
BT601 = {
    "to_rgb": {"y": 0.00456621, "rv": 0.00625893, "gu": -0.00153632, "gv": -0.00318811, "bu": 0.00791071,
               "offset": (-222.921, 135.576, -276.836)},
    "to_ycbcr": {"y": (65.481, 128.553, 24.966), "cb": (-37.797, -74.203, 112.0), "cr": (112.0, -93.786, -18.214),
                 "offset": (16.0, 128.0, 128.0)},
}


# The colour spaces of `colour=`, in the order of their integer id in the C ABI (SAVSR_YUV_*): name -> (Kr, Kb, full range).  "bt601" is
# the BT601 table above as it stands (its constants are rounded, so it is not rebuilt from Kr, Kb); "bt601-full" is JFIF's exact form.
COLOURS = ("bt601", "bt709", "bt601-full", "bt709-full")
_SPACES = {"bt709": (0.2126, 0.0722, False), "bt601-full": (0.299, 0.114, True), "bt709-full": (0.2126, 0.0722, True)}


def check_colour(colour, what: str = "colour") -> int:
    """The id of a colour space name (its position in COLOURS); refuses anything else, naming the list."""
    if not isinstance(colour, str) or colour not in COLOURS:
        raise ValueError(f"{what} = {colour!r}: one of {', '.join(COLOURS)}")
    return COLOURS.index(colour)


def is_full_range(colour: str) -> bool:
    return colour != "bt601" and _SPACES[COLOURS[check_colour(colour)]][2]


def _build(kr: float, kb: float, full: bool) -> dict:
    """A table of BT601's shape from the luma weights and the range, in float64.  With Kg = 1 - Kr - Kb, Y' = Kr R + Kg G + Kb B,
    Cb = (B - Y') / (2 (1 - Kb)), Cr = (R - Y') / (2 (1 - Kr)); 8-bit samples Y = oy + sy Y', C = 128 + sc C'  (limited: sy = 219,
    oy = 16, sc = 224; full: sy = 255, oy = 0, sc = 255).  Every entry is the expression below as written, evaluated left to right
    inside its parentheses: make_matrix in yuv.hip evaluates the same ones, so that the two tables agree to the last bit."""
    sy, oy, sc = (255.0, 0.0, 255.0) if full else (219.0, 16.0, 224.0)
    kg = (1.0 - kr) - kb
    db, dr = 2.0 * (1.0 - kb), 2.0 * (1.0 - kr)
    y = 1.0 / sy
    rv = dr / sc
    gu = -((db * kb) / (kg * sc))
    gv = -((dr * kr) / (kg * sc))
    bu = db / sc
    base = -(oy * y)
    return {
        "to_rgb": {"y": y, "rv": rv, "gu": gu, "gv": gv, "bu": bu,
                   "offset": ((base - 128.0 * rv) * 255.0, ((base - 128.0 * gu) - 128.0 * gv) * 255.0, (base - 128.0 * bu) * 255.0)},
        "to_ycbcr": {"y": (sy * kr, sy * kg, sy * kb),
                     "cb": (-((sc * kr) / db), -((sc * kg) / db), sc * 0.5),
                     "cr": (sc * 0.5, -((sc * kg) / dr), -((sc * kb) / dr)),
                     "offset": (oy, 128.0, 128.0)},
    }


_MATRICES = {"bt601": BT601}


def matrix(colour: str = "bt601") -> dict:
    """The coefficient table of a colour space, of BT601's shape: BT601 itself for "bt601", `_build` of (Kr, Kb, range) otherwise."""
    name = COLOURS[check_colour(colour)]
    if name not in _MATRICES:
        _MATRICES[name] = _build(*_SPACES[name])
    return _MATRICES[name]


DEPTHS = (8, 10, 12)


def check_depth(depth, what: str = "depth") -> int:
    """A bit depth as an int; refuses anything but 8, 10 and 12, naming the list."""
    if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or int(depth) not in DEPTHS:
        raise ValueError(f"{what} = {depth!r}: one of {', '.join(str(d) for d in DEPTHS)}")
    return int(depth)


def check_depth_colour(depth, colour: str, what: str = "depth", cwhat: str = "colour") -> int:
    """check_depth, and the rule that 10 and 12 bits are defined for the limited-range colour spaces only."""
    d = check_depth(depth, what)
    if d > 8 and is_full_range(colour):
        raise ValueError(f"{what} = {d} with {cwhat} = {colour!r}: 10 and 12 bits are defined for limited range only (bt601, bt709); "
                         f"full range at depth d scales by 2^d - 1 and is not implemented")
    return d


# The chroma layouts of `chroma=`, in the order of their integer id in the C ABI (SAVSR_CHROMA_*), and the pixel format / output kind
# each one goes by in the public interface.
CHROMAS = ("420", "422", "444")
FORMAT_OF = {"420": "i420", "422": "i422", "444": "i444"}
CHROMA_OF = {v: k for k, v in FORMAT_OF.items()}


def check_chroma(chroma, what: str = "chroma") -> int:
    """The id of a chroma layout name (its position in CHROMAS); refuses anything else, naming the list."""
    if not isinstance(chroma, str) or chroma not in CHROMAS:
        raise ValueError(f"{what} = {chroma!r}: one of {', '.join(CHROMAS)}")
    return CHROMAS.index(chroma)


def chroma_hw(h: int, w: int, chroma: str = "420") -> Tuple[int, int]:
    """(ch, cw) of a chroma plane: both halved (rounded up) in 4:2:0, the width alone in 4:2:2, neither in 4:4:4."""
    if chroma == "420":
        return (h + 1) // 2, (w + 1) // 2
    return (h, (w + 1) // 2) if CHROMAS[check_chroma(chroma)] == "422" else (h, w)


# The chroma sitings of `siting=`; the id of the C ABI (SAVSR_SITING_*) is the position plus one, 0 (None) = not modelled.
SITINGS = ("centre", "left", "topleft")


def check_siting(siting, chroma: str = "420", what: str = "siting") -> int:
    """The C-ABI id of a siting: 0 for None, the position in SITINGS plus one otherwise; refuses anything else, naming the list, and
    "topleft" with 4:2:2, naming the rule."""
    if siting is None:
        return 0
    if not isinstance(siting, str) or siting not in SITINGS:
        raise ValueError(f"{what} = {siting!r}: None or one of {', '.join(SITINGS)}")
    if siting == "topleft" and CHROMAS[check_chroma(chroma)] == "422":
        raise ValueError(f"{what} = 'topleft' with 4:2:2 chroma: 4:2:2 has no vertical subsampling; its cosited form is 'left'")
    return SITINGS.index(siting) + 1


def frame_bytes(h: int, w: int, depth: int = 8, chroma: str = "420") -> int:
    """Bytes of a frame in the given layout: a byte per sample at 8 bits, a 16-bit word at 10 and 12.  chroma = "400" (MONO): the Y plane
    alone, a grey-scale frame (the module's "Luma-only checkpoints")."""
    if chroma == MONO:
        return h * w * (1 if depth == 8 else 2)
    ch, cw = chroma_hw(h, w, chroma)
    return (h * w + 2 * ch * cw) * (1 if depth == 8 else 2)


def i420_bytes(h: int, w: int, depth: int = 8) -> int:
    """Bytes of a 4:2:0 frame: frame_bytes of the default layout."""
    return frame_bytes(h, w, depth)


def layout_name(chroma: str) -> str:
    """What the messages call a frame of the layout: I420, I422, I444; Y400 for grey-scale frames (MONO)."""
    return "Y400" if chroma == MONO else "I" + chroma


def _check_size(h: int, w: int) -> None:
    if int(h) != h or int(w) != w or h < 1 or w < 1:
        raise ValueError(f"size must be (h, w) with h, w >= 1, got ({h!r}, {w!r})")


def split_planes(frames: np.ndarray, h: int, w: int, depth: int = 8, chroma: str = "420") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """[N, frame_bytes(h, w, depth, chroma)] uint8 -> Y [N, h, w], U [N, ch, cw], V [N, ch, cw]: uint8 views at 8 bits, the little-endian
    16-bit samples as uint16 arrays at 10 and 12."""
    _check_size(h, w)
    check_chroma(chroma)
    frames = np.asarray(frames)
    fb, name = frame_bytes(h, w, depth, chroma), layout_name(chroma)
    if depth != 8:
        depth = check_depth(depth)
        if frames.dtype != np.uint8 or frames.ndim != 2 or frames.shape[1] != fb:
            raise ValueError(f"{depth}-bit {name} frames of {h} x {w} are [N, {fb}] uint8, got {frames.dtype} {tuple(frames.shape)}")
        frames = np.ascontiguousarray(frames).view("<u2")
    elif frames.dtype != np.uint8 or frames.ndim != 2 or frames.shape[1] != fb:
        raise ValueError(f"{name} frames of {h} x {w} are [N, {fb}] uint8, got {frames.dtype} {tuple(frames.shape)}")
    ch, cw = chroma_hw(h, w, chroma)
    n = frames.shape[0]
    y = frames[:, :h * w].reshape(n, h, w)
    u = frames[:, h * w:h * w + ch * cw].reshape(n, ch, cw)
    v = frames[:, h * w + ch * cw:].reshape(n, ch, cw)
    return y, u, v


def to_rgb_tables(m: dict = BT601) -> dict:
    """The five per-sample float32 tables of i420_to_rgb: "y" (no offset) and the four chroma terms, each with its channel's offset
    folded in (R's in "rv", G's in "gu", B's in "bu").  float64 product and sum, one rounding to float32."""
    t = m["to_rgb"]
    s = np.arange(256, dtype=np.float64)
    o = [v / 255.0 for v in t["offset"]]
    return {"y": (s * t["y"]).astype(np.float32),
            "rv": (s * t["rv"] + o[0]).astype(np.float32),
            "gu": (s * t["gu"] + o[1]).astype(np.float32),
            "gv": (s * t["gv"]).astype(np.float32),
            "bu": (s * t["bu"] + o[2]).astype(np.float32)}


def to_rgb_coefficients(colour: str, depth: int) -> dict:
    """The float32 constants of the high-depth i420_to_rgb: the five to-RGB entries divided by k = 2^(depth - 8) (exact) and the three
    offsets / 255, each rounded once to float32."""
    t = matrix(colour)["to_rgb"]
    k = float(1 << (check_depth_colour(depth, colour) - 8))
    c = {name: np.float32(t[name] / k) for name in ("y", "rv", "gu", "gv", "bu")}
    c["offset"] = tuple(np.float32(v / 255.0) for v in t["offset"])
    return c


def replicate_chroma(p: np.ndarray, h: int, w: int, chroma: str = "420") -> np.ndarray:
    """A chroma plane [N, ch, cw] -> [N, h, w] by nearest replication over the layout's block: 2 x 2, 1 x 2, or the plane itself."""
    if chroma == "444":
        return p
    if chroma == "422":
        return np.repeat(p, 2, axis=2)[:, :, :w]
    return np.repeat(np.repeat(p, 2, axis=1), 2, axis=2)[:, :h, :w]


def _lerp_axis(c: np.ndarray, n: int, axis: int, cosited: bool) -> np.ndarray:
    """Integer numerators over 4 of the linear interpolation along one subsampled axis, ceil(n / 2) samples -> n pixels, the edge samples
    replicated.  Pixel 2 c: 3 C[c] + C[c - 1] (centre), 4 C[c] (cosited); pixel 2 c + 1: 3 C[c] + C[c + 1], 2 C[c] + 2 C[c + 1]."""
    nc = c.shape[axis]
    i = np.arange(n) // 2
    odd = (np.arange(n) % 2).astype(bool)
    cur = np.take(c, i, axis)
    shape = [1] * c.ndim
    shape[axis] = n
    odd = odd.reshape(shape)
    nxt = np.take(c, np.minimum(i + 1, nc - 1), axis)
    if cosited:
        return np.where(odd, 2 * cur + 2 * nxt, 4 * cur)
    prv = np.take(c, np.maximum(i - 1, 0), axis)
    return 3 * cur + np.where(odd, nxt, prv)


def interpolate_chroma(plane: np.ndarray, h: int, w: int, chroma: str, siting: str) -> np.ndarray:
    """A chroma plane [N, ch, cw] of integer samples -> float32 [N, h, w]: the chroma at every luma pixel under the siting (the module's
    "Chroma siting"), an integer numerator times 2^-4 (4:2:0) or 2^-2 (4:2:2), exact.  4:4:4: the plane's own values."""
    sid = check_siting(siting, chroma)
    if sid == 0:
        raise ValueError(f"siting = None models no siting: one of {', '.join(SITINGS)} (replicate_chroma is the nearest reading)")
    p = np.asarray(plane).astype(np.int64)
    if p.ndim != 3 or p.shape[1:] != chroma_hw(h, w, chroma):
        raise ValueError(f"a {layout_name(chroma)} chroma plane of {h} x {w} is [N, {', '.join(str(v) for v in chroma_hw(h, w, chroma))}], got {tuple(p.shape)}")
    if chroma == "444":
        return p.astype(np.float32)
    num = _lerp_axis(p, w, 2, siting != "centre")
    if chroma == "422":
        return num.astype(np.float32) * np.float32(0.25)
    return _lerp_axis(num, h, 1, siting == "topleft").astype(np.float32) * np.float32(0.0625)


def _full_planes(frames_u8: np.ndarray, h: int, w: int, depth: int, chroma: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """split_planes with both chroma planes replicated to [N, h, w]."""
    y, u, v = split_planes(frames_u8, h, w, depth, chroma)
    return y, replicate_chroma(u, h, w, chroma), replicate_chroma(v, h, w, chroma)


def _stack01(r: np.ndarray, g: np.ndarray, b: np.ndarray) -> np.ndarray:
    out = np.stack([r, g, b], 1)
    return np.fmin(np.fmax(out, np.float32(0.0)), np.float32(1.0)).astype(np.float32)


def _i420_to_rgb_16(frames_u8: np.ndarray, h: int, w: int, colour: str, depth: int, chroma: str = "420") -> np.ndarray:
    c = to_rgb_coefficients(colour, depth)
    top = np.uint16((1 << depth) - 1)
    y, u, v = (np.minimum(p, top).astype(np.float32) for p in _full_planes(frames_u8, h, w, depth, chroma))
    yt = y * c["y"]
    r = (yt + v * c["rv"]) + c["offset"][0]
    g = ((yt + u * c["gu"]) + v * c["gv"]) + c["offset"][1]
    b = (yt + u * c["bu"]) + c["offset"][2]
    return _stack01(r, g, b)


def _i420_to_rgb_sited(frames_u8: np.ndarray, h: int, w: int, colour: str, depth: int, chroma: str, siting: str) -> np.ndarray:
    """The coefficient arithmetic of _i420_to_rgb_16 at any depth on linearly interpolated chroma."""
    c = to_rgb_coefficients(colour, depth)
    top = (1 << depth) - 1
    y, u, v = (np.minimum(p, top) for p in split_planes(frames_u8, h, w, depth, chroma))
    y = y.astype(np.float32)
    u, v = interpolate_chroma(u, h, w, chroma, siting), interpolate_chroma(v, h, w, chroma, siting)
    yt = y * c["y"]
    r = (yt + v * c["rv"]) + c["offset"][0]
    g = ((yt + u * c["gu"]) + v * c["gv"]) + c["offset"][1]
    b = (yt + u * c["bu"]) + c["offset"][2]
    return _stack01(r, g, b)


def i420_to_rgb(frames_u8: np.ndarray, h: int, w: int, colour: str = "bt601", depth: int = 8, chroma: str = "420", siting=None) -> np.ndarray:
    """[N, frame_bytes(h, w, depth, chroma)] uint8 -> float32 [N, 3, h, w] in [0, 1].  depth = 8:  R = y + rv,  G = (y + gu) + gv,
    B = y + bu  on the table values; 10 and 12: float32 arithmetic on the samples (the module's "High depth").  chroma: the layout
    (the module's "Chroma layouts"); the default is I420.  siting: None (nearest replication, the lines above) or one of SITINGS: chroma
    interpolated linearly at the siting's positions, then the coefficient arithmetic at every depth (the module's "Chroma siting")."""
    if check_siting(siting, chroma) and chroma != "444":
        return _i420_to_rgb_sited(frames_u8, h, w, colour, check_depth(depth), chroma, siting)
    if depth != 8:
        return _i420_to_rgb_16(frames_u8, h, w, colour, depth, chroma)
    y, u, v = _full_planes(frames_u8, h, w, 8, chroma)
    t = to_rgb_tables(matrix(colour))
    ty = t["y"][y]
    r = ty + t["rv"][v]
    g = (ty + t["gu"][u]) + t["gv"][v]
    b = ty + t["bu"][u]
    return _stack01(r, g, b)


def _clamp01(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim != 4 or x.shape[1] != 3:
        raise ValueError(f"RGB frames are [N, 3, H, W] float32, got {x.dtype} {tuple(x.shape)}")
    return np.fmin(np.fmax(x, np.float32(0.0)), np.float32(1.0))      # (fmaxf / fminf: a NaN becomes 0)


def _row(p: np.ndarray, coef, offset: float) -> np.ndarray:
    """((r * a + g * b) + b * c) + offset in float32, every product and sum rounded."""
    a, b, c = (np.float32(v) for v in coef)
    return ((p[:, 0] * a + p[:, 1] * b) + p[:, 2] * c) + np.float32(offset)


def _block_mean(p: np.ndarray, chroma: str = "420") -> np.ndarray:
    """Mean of every 2 x 2 block's in-image pixels, [N, 3, H, W] -> [N, 3, ch, cw]:  ((a + b) + (c + d)) * 0.25 with a b the block's
    upper row and c d its lower; (a + b) * 0.5 for a pair (the last row of an odd H, the last column of an odd W); the pixel alone.
    4:2:2: (a + b) * 0.5 over a row's pairs, the pixel alone in the last column of an odd W.  4:4:4: the pixels themselves."""
    n, c, H, W = p.shape
    if chroma == "444":
        return p
    if chroma == "422":
        we = W // 2 * 2
        m = np.empty((n, c, H, (W + 1) // 2), np.float32)
        m[:, :, :, :W // 2] = (p[:, :, :, 0:we:2] + p[:, :, :, 1:we:2]) * np.float32(0.5)
        if W % 2:
            m[:, :, :, -1] = p[:, :, :, W - 1]
        return m
    ch, cw = chroma_hw(H, W)
    he, we = H // 2 * 2, W // 2 * 2
    m = np.empty((n, c, ch, cw), np.float32)
    m[:, :, :H // 2, :W // 2] = ((p[:, :, 0:he:2, 0:we:2] + p[:, :, 0:he:2, 1:we:2]) +
                                 (p[:, :, 1:he:2, 0:we:2] + p[:, :, 1:he:2, 1:we:2])) * np.float32(0.25)
    if W % 2:
        m[:, :, :H // 2, -1] = (p[:, :, 0:he:2, W - 1] + p[:, :, 1:he:2, W - 1]) * np.float32(0.5)
    if H % 2:
        m[:, :, -1, :W // 2] = (p[:, :, H - 1, 0:we:2] + p[:, :, H - 1, 1:we:2]) * np.float32(0.5)
    if W % 2 and H % 2:
        m[:, :, -1, -1] = p[:, :, H - 1, W - 1]
    return m


def _h3(l: np.ndarray, c: np.ndarray, r: np.ndarray) -> np.ndarray:
    """[1 2 1] / 4 in float32: ((l + r) + (c + c)) * 0.25."""
    return ((l + r) + (c + c)) * np.float32(0.25)


def filter_chroma_rgb(p: np.ndarray, chroma: str = "420", siting=None) -> np.ndarray:
    """The RGB a chroma sample is computed from, [N, 3, H, W] float32 (clamped) -> [N, 3, ch, cw]: `_block_mean` for None and "centre"
    (the box is the centre-sited filter), [1 2 1] / 4 with clamped taps along every cosited axis (the module's "Chroma siting")."""
    sid = check_siting(siting, chroma)
    if chroma == "444" or sid < 2:
        return _block_mean(p, chroma)
    p = np.asarray(p)
    if p.dtype != np.float32 or p.ndim != 4:
        raise ValueError(f"RGB frames are [N, 3, H, W] float32, got {p.dtype} {tuple(p.shape)}")
    H, W = p.shape[2:]
    ch, cw = chroma_hw(H, W, chroma)
    xs = 2 * np.arange(cw)
    hr = _h3(p[:, :, :, np.maximum(xs - 1, 0)], p[:, :, :, xs], p[:, :, :, np.minimum(xs + 1, W - 1)])          # Hrow of every row
    if chroma == "422":
        return hr
    ys = 2 * np.arange(ch)
    if siting == "topleft":
        return _h3(hr[:, :, np.maximum(ys - 1, 0)], hr[:, :, ys], hr[:, :, np.minimum(ys + 1, H - 1)])
    m = np.empty(hr.shape[:2] + (ch, cw), np.float32)
    m[:, :, :H // 2] = (hr[:, :, 0:H // 2 * 2:2] + hr[:, :, 1:H // 2 * 2:2]) * np.float32(0.5)
    if H % 2:
        m[:, :, -1] = hr[:, :, H - 1]
    return m


def ycbcr_f32(x: np.ndarray, colour: str = "bt601", chroma: str = "420", siting=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The float32 values rgb_to_i420 rounds: Y [N, H, W], Cb and Cr [N, ch, cw], in 8-bit steps.  siting: where the chroma samples lie
    (filter_chroma_rgb); None and "centre" are the block mean."""
    check_chroma(chroma)
    p = _clamp01(x)
    t = matrix(colour)["to_ycbcr"]
    m = filter_chroma_rgb(p, chroma, siting)
    return _row(p, t["y"], t["offset"][0]), _row(m, t["cb"], t["offset"][1]), _row(m, t["cr"], t["offset"][2])


def rgb_to_i420(x_f32: np.ndarray, colour: str = "bt601", depth: int = 8, chroma: str = "420", siting=None, dither=None) -> np.ndarray:
    """float32 [N, 3, H, W] -> uint8 [N, frame_bytes(H, W, depth, chroma)].  Limited range: after the clamp Y lies in 16 .. 235 and
    chroma in 16 .. 240, no clip.  Full range: chroma reaches 255.5, which rounds to 256, so the rounded values are clipped to 0 .. 255.
    depth = 10, 12 (limited range only): rint(ycbcr_f32 * 2^(depth - 8)), written as little-endian 16-bit samples.  chroma: the layout
    (the module's "Chroma layouts"); the default is I420.  siting: where the chroma samples lie (the module's "Chroma siting"); None and
    "centre" are the block mean.  dither: None (rint, the lines above) or one of dither.DITHERS: floor(t + theta) in place of rint(t) in
    every plane, theta at the sample's own coordinates in its plane (savsr_amd/dither.py; savsr_video_quantize_yuvs_d)."""
    rnd = np.rint if check_dither(dither) is None else dither_floor
    if depth != 8:
        k = np.float32(1 << (check_depth_colour(depth, colour) - 8))
        planes = [rnd(v * k) for v in ycbcr_f32(x_f32, colour, chroma, siting)]
    else:
        planes = [rnd(v) for v in ycbcr_f32(x_f32, colour, chroma, siting)]
        if is_full_range(colour):
            planes = [np.fmin(np.fmax(v, np.float32(0.0)), np.float32(255.0)) for v in planes]
    n = planes[0].shape[0]
    return np.concatenate([v.astype(np.uint8 if depth == 8 else "<u2").reshape(n, -1) for v in planes], 1).view(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------
# Luma-only checkpoints (num_in_ch = 1) on YUV and grey-scale video: the specification of luma.hip -- savsr_video_gather_luma,
# savsr_video_quantize_luma and savsr_video_resample_chroma -- and of upscale_video(chroma_filter="bicubic").  Y goes through the network,
# Cb / Cr go from samples to samples through a separable, siting-aware Keys cubic at the network's scale.
#
#   luma in    min(s, 2^d - 1) as float32, divided by float32(255 k), k = 2^(d - 8): one IEEE float32 division.  A Y-only model is trained
#              on Y / 255 of limited-range codes (rgb2ycbcr(y_only=True)); the same rule is applied whatever the colour id -- the colour
#              space is documented, not converted (a luma-only network never forms RGB).  At 8 bits: savsr_video_gather_u8's value.
#   luma out   rint(clamp(v, 0, 1) * float32(255 k)), half to even, NaN -> 0.  At 8 bits: savsr_video_quantize_u8's rule.
#   chroma     `chroma_axis_table` per axis, then `resample_chroma`: width first, then height, float32 in tap order without fused
#              multiply-add, x 2^(D - d), rint, clip to 0 .. 2^D - 1 (the cubic overshoots).
#
# MONO = "400" is the layout of a grey-scale frame (Y4M's Cmono): the Y plane alone.
MONO = "400"
LUMA_FORMAT = "y400"
CHROMA_FILTERS = ("bicubic",)
_SUB = {"420": (2, 2), "422": (1, 2), "444": (1, 1)}          # (vertical, horizontal) luma samples per chroma sample


def check_chroma_filter(chroma_filter) -> None:
    """chroma_filter is None or one of CHROMA_FILTERS; refuses anything else, naming the list."""
    if chroma_filter is not None and (not isinstance(chroma_filter, str) or chroma_filter not in CHROMA_FILTERS):
        raise ValueError(f"chroma_filter = {chroma_filter!r}: None or one of {', '.join(CHROMA_FILTERS)}")


def subsampling(chroma: str) -> Tuple[int, int]:
    """(vertical, horizontal) luma samples per chroma sample of a layout: (2, 2), (1, 2), (1, 1)."""
    return _SUB[CHROMAS[check_chroma(chroma)]]


def luma_to_unit(samples: np.ndarray, depth: int = 8) -> np.ndarray:
    """Y samples -> the float32 values a luma-only network reads: float32(min(s, 2^d - 1)) / float32(255 * 2^(d - 8))."""
    d = check_depth(depth)
    s = np.minimum(np.asarray(samples).astype(np.int64), (1 << d) - 1).astype(np.float32)
    return s / np.float32(255 << (d - 8))


def unit_to_luma(v: np.ndarray, depth: int = 8, dither=None) -> np.ndarray:
    """The network's float32 luma -> Y samples (uint8 at 8 bits, uint16 at 10 / 12): rint(clamp(v, 0, 1) * float32(255 * 2^(d - 8))),
    half to even; fmax / fmin, so a NaN becomes 0.  dither: None or one of dither.DITHERS: floor(t + theta) in place of rint(t), theta at
    the sample's (y, x) in the last two axes (savsr_amd/dither.py; savsr_video_quantize_luma_d)."""
    d = check_depth(depth)
    v = np.asarray(v, dtype=np.float32)
    rnd = np.rint if check_dither(dither) is None else dither_floor
    q = rnd(np.fmin(np.fmax(v, np.float32(0.0)), np.float32(1.0)) * np.float32(255 << (d - 8)))
    return q.astype(np.uint8 if d == 8 else np.uint16)


def _cosited(siting, axis: str) -> bool:
    """Whether a siting puts the chroma samples on luma samples along an axis: "left" and "topleft" along x, "topleft" along y."""
    if siting is not None and (not isinstance(siting, str) or siting not in SITINGS):
        raise ValueError(f"siting = {siting!r}: None or one of {', '.join(SITINGS)}")
    if axis not in ("x", "y"):
        raise ValueError(f"axis = {axis!r}: 'x' or 'y'")
    return siting == "topleft" or (siting == "left" and axis == "x")


def _keys(x: np.ndarray) -> np.ndarray:
    """The Keys cubic with a = -0.5, float64."""
    ax = np.abs(x)
    ax2, ax3 = ax * ax, ax * ax * ax
    a = -0.5
    return np.where(ax <= 1, (a + 2) * ax3 - (a + 3) * ax2 + 1, np.where(ax <= 2, a * ax3 - 5 * a * ax2 + 8 * a * ax - 4 * a, 0.0))


def chroma_axis_table(n_in_luma: int, n_out_luma: int, sub_in: int, sub_out: int, siting_in=None, siting_out=None, axis: str = "x"):
    """(xmin[int32], xsize[int32], weights[float32][max_taps]) of one axis of the chroma resampler: ceil(n_in_luma / sub_in) input samples
    -> ceil(n_out_luma / sub_out) output samples.  Output sample j lies at HR luma position P = sub_out j + o_out, input sample c at LR
    luma position sub_in c + o_in, o = (sub - 1) / 2 for a centre-sited or unmodelled (None) axis and 0 for a cosited one (`axis` says
    which axis of the siting this is): interpolate_chroma's positions.  The luma grids are related by pixel centres and the actual sizes,
    p = (P + 0.5) n_in_luma / n_out_luma - 0.5, so the position among the input samples is u = (p - o_in) / sub_in.  With
    rho = sub_out n_in_luma / (n_out_luma sub_in) input samples per output sample and aa = min(1, 1 / rho): the Keys cubic (a = -0.5) of
    (u - tap) aa over ceil(4 / aa) + 2 taps from floor(u) - ksize // 2 + 1, normalised to sum 1; taps outside the plane fold onto the
    pixels inside by core.py's border rule (-1 -> 0, -2 -> 1, n -> n - 1; applied again where a plane is shorter than the reach):
    resize_gpu.core_tables with a general position.  float64 throughout, each folded weight rounded to float32 once; taps of weight 0
    at either end of a window are dropped, so an axis with u == j exactly gives the single weight 1.0."""
    for v in (n_in_luma, n_out_luma):
        if int(v) != v or v < 1:
            raise ValueError(f"luma sizes must be integers >= 1, got ({n_in_luma!r}, {n_out_luma!r})")
    if sub_in not in (1, 2) or sub_out not in (1, 2):
        raise ValueError(f"sub_in, sub_out = {sub_in!r}, {sub_out!r}: 1 or 2 luma samples per chroma sample")
    n_in_luma, n_out_luma = int(n_in_luma), int(n_out_luma)
    o_in = 0.0 if _cosited(siting_in, axis) else (sub_in - 1) / 2.0
    o_out = 0.0 if _cosited(siting_out, axis) else (sub_out - 1) / 2.0
    n_in, n_out = -(-n_in_luma // sub_in), -(-n_out_luma // sub_out)
    rho = (sub_out * n_in_luma) / (n_out_luma * sub_in)
    aa = min(1.0, 1.0 / rho)
    ksize = int(np.ceil(4.0 / aa)) + 2
    rows, xmin, xsize = [], np.zeros(n_out, np.int32), np.zeros(n_out, np.int32)
    for j in range(n_out):
        p = ((sub_out * j + o_out) + 0.5) * n_in_luma / n_out_luma - 0.5
        u = (p - o_in) / sub_in
        base = int(np.floor(u)) - ksize // 2 + 1
        taps = base + np.arange(ksize)
        wt = _keys((u - taps) * aa)
        wt = wt / wt.sum()
        folded = np.zeros(n_in, np.float64)
        for t, v in zip(taps, wt):
            t = int(t)
            while t < 0 or t >= n_in:
                t = -t - 1 if t < 0 else 2 * n_in - 1 - t
            folded[t] += v
        nz = np.nonzero(folded)[0]
        lo, hi = int(nz[0]), int(nz[-1])
        xmin[j], xsize[j] = lo, hi - lo + 1
        rows.append(folded[lo:hi + 1].astype(np.float32))
    weights = np.zeros((n_out, int(xsize.max())), np.float32)
    for j, r in enumerate(rows):
        weights[j, :len(r)] = r
    return xmin, xsize, weights


def chroma_tables(h: int, w: int, H: int, W: int, chroma: str, out_chroma: str, siting=None, out_siting=None):
    """(table_y, table_x) of `chroma_axis_table` for an h x w -> H x W picture and the two layouts and sitings."""
    check_siting(siting, chroma, "siting")
    check_siting(out_siting, out_chroma, "out_siting")
    (sy, sx), (oy, ox) = subsampling(chroma), subsampling(out_chroma)
    return (chroma_axis_table(h, H, sy, oy, siting, out_siting, "y"), chroma_axis_table(w, W, sx, ox, siting, out_siting, "x"))


def dense_axis(table, n_in: int) -> np.ndarray:
    """The [out][in] float32 matrix of an axis table."""
    xmin, xsize, wt = table
    m = np.zeros((len(xmin), n_in), np.float32)
    for j in range(len(xmin)):
        m[j, xmin[j]:xmin[j] + xsize[j]] = wt[j, :xsize[j]]
    return m


def _filter_axis(x: np.ndarray, table, axis: int) -> np.ndarray:
    """acc = w0 s0, then acc = acc + wi si in tap order, float32, every product and sum rounded; taps beyond an output's xsize skipped."""
    xmin, xsize, wt = table
    shape = [1] * x.ndim
    shape[axis] = len(xmin)
    n = x.shape[axis]
    acc = None
    for t in range(wt.shape[1]):
        prod = wt[:, t].reshape(shape) * np.take(x, np.minimum(xmin + t, n - 1), axis)
        acc = prod if acc is None else np.where((t < xsize).reshape(shape), acc + prod, acc)
    return acc.astype(np.float32)


def resample_chroma(plane: np.ndarray, table_y, table_x, depth_in: int = 8, depth_out: int = 8) -> np.ndarray:
    """Chroma samples [..., ch, cw] -> [..., cH, cW] (uint8 at depth_out = 8, uint16 at 10 / 12): samples clipped to 2^d - 1; the width
    through table_x, then the height through table_y over the filtered rows (`_filter_axis`); x 2^(D - d) (exact); rint, half to even;
    clipped to 0 .. 2^D - 1."""
    d, D = check_depth(depth_in, "depth_in"), check_depth(depth_out, "depth_out")
    p = np.asarray(plane)
    if p.ndim < 2 or not np.issubdtype(p.dtype, np.integer):
        raise ValueError(f"a chroma plane is [..., ch, cw] of integer samples, got {p.dtype} {tuple(p.shape)}")
    s = np.minimum(p.astype(np.int64), (1 << d) - 1).astype(np.float32)
    v = _filter_axis(_filter_axis(s, table_x, s.ndim - 1), table_y, s.ndim - 2)
    v = np.rint(v * np.float32(2.0 ** (D - d)))
    v = np.fmin(np.fmax(v, np.float32(0.0)), np.float32((1 << D) - 1))
    return v.astype(np.uint8 if D == 8 else np.uint16)


def luma_plane(frames: np.ndarray, h: int, w: int, depth: int = 8, chroma: str = "420") -> np.ndarray:
    """The Y samples [N, h, w] of frames [N, frame_bytes(h, w, depth, chroma)] uint8 (chroma = MONO: grey-scale frames)."""
    frames = np.asarray(frames)
    fb = frame_bytes(h, w, check_depth(depth), chroma)
    if frames.dtype != np.uint8 or frames.ndim != 2 or frames.shape[1] != fb:
        raise ValueError(f"frames of {h} x {w} are [N, {fb}] uint8, got {frames.dtype} {tuple(frames.shape)}")
    s = 1 if depth == 8 else 2
    y = np.ascontiguousarray(frames[:, :h * w * s])
    return (y if depth == 8 else y.view("<u2")).reshape(frames.shape[0], h, w)


def luma_only_frames(frames: np.ndarray, h: int, w: int, sr_luma_unit: np.ndarray, depth: int = 8, out_depth=None, chroma: str = "420",
                     out_chroma=None, siting=None, out_siting=None) -> np.ndarray:
    """The output frames of a luma-only network on YUV video: frames [N, frame_bytes(h, w, depth, chroma)] uint8 and the network's
    float32 luma [N, 1, H, W] (or [N, H, W]) -> uint8 [N, frame_bytes(H, W, out_depth, out_chroma)].  Y = unit_to_luma of the network's
    result; U and V = resample_chroma of the same input frame's planes.  out_chroma = MONO drops the chroma; chroma = MONO has none to
    give, so only MONO comes out of it."""
    D = check_depth(depth if out_depth is None else out_depth, "out_depth")
    out_chroma = chroma if out_chroma is None else out_chroma
    sr = np.asarray(sr_luma_unit, dtype=np.float32)
    if sr.ndim == 4 and sr.shape[1] == 1:
        sr = sr[:, 0]
    n = np.asarray(frames).shape[0]
    if sr.ndim != 3 or sr.shape[0] != n:
        raise ValueError(f"the network's luma is [N, 1, H, W] float32 for N = {n} frames, got {tuple(np.asarray(sr_luma_unit).shape)}")
    H, W = sr.shape[1:]
    planes = [unit_to_luma(sr, D)]
    if out_chroma != MONO:
        if chroma == MONO:
            raise ValueError(f"grey-scale frames have no chroma planes: out_chroma = {out_chroma!r} cannot be made from them")
        ty, tx = chroma_tables(h, w, H, W, chroma, out_chroma, siting, out_siting)
        _, u, v = split_planes(frames, h, w, depth, chroma)
        planes += [resample_chroma(u, ty, tx, depth, D), resample_chroma(v, ty, tx, depth, D)]
    else:
        luma_plane(frames, h, w, depth, chroma)          # (the shape check)
    return np.concatenate([np.ascontiguousarray(q.astype(np.uint8 if D == 8 else "<u2")).reshape(n, -1).view(np.uint8) for q in planes], 1)
