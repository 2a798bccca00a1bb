"""The active picture of letterboxed video: the host-side specification (numpy / pure Python, no GPU needed).

A letterboxed, pillarboxed or window-boxed video carries hard-matted black bars.  `upscale_video(v, crop=R, ...)` is, bit for bit,
`upscale_video` on the video cropped to the rect R = (y0, x0, ah, aw) by hand (`crop_frames`) with every other argument the same; with
bars="keep" that result is put back into a full-size frame of nominal black (`place`, `insert_frames`).  The crop comes before anything
else looks at the video, so the cuts, the windows, the self-ensemble, fp16 and the luma-only path all see the cropped video.

The detector: per frame the sum of the 8-bit samples of every row and of every column (`line_sums`, the specification of
savsr_video_line_sums_u8 / _u16 / _f32 in csrc/active.hip), the largest sum of every line over the frames, then ffmpeg cropdetect's rule in
exact arithmetic (`active_rect`): a line whose mean is at most `limit` is black, and the picture spans the first to the last line that is
not.  The default limit is cropdetect's, 24 on the 8-bit scale; it is a parameter and is not validated on real footage here.
`align_rect` moves a detected rect's offsets outwards to the chroma block of the input layout; an explicit rect must sit there already
(`check_rect`).
"""
from __future__ import annotations

import math
from fractions import Fraction
from typing import Optional, Sequence, Tuple

import numpy as np

from .packing import get_hw
from .frames import SAMPLE_FORMATS, block_of, check_pixel_format, layout_of          # (block_of: the chroma blocks live with the plane table)
from .scenes import _samples_of
from .yuv import MONO, check_depth, chroma_hw, frame_bytes, is_full_range, luma_plane, split_planes

Rect = Tuple[int, int, int, int]
BARS = ("keep", "drop")
DEFAULT_LIMIT = 24          # ffmpeg cropdetect's default, on the 8-bit scale; not validated on real footage


# ---- the detector --------------------------------------------------------------------------------------------------------------------
def line_sums(frames, pixel_format: str = "rgb", size=None, depth: int = 8) -> Tuple[np.ndarray, np.ndarray]:
    """(rows [N, h] int64, cols [N, w] int64): per frame the sum of the 8-bit samples of every row and of every column; the samples are
    the ones scenes.pair_sad compares.  [N, h, w, c] uint8: every byte (a row holds c * w samples, a column c * h).  Planar frames (i420,
    i422, i444, y400 with size=): the Y plane only (w and h samples); at 10 or 12 bits every sample as its 8 most significant bits,
    min(s, 2^d - 1) >> (d - 8).  [N, c, h, w] float: every value after scenes.quantize_u8, summed over the channels."""
    hw = check_pixel_format(pixel_format, size)
    if hasattr(frames, "detach"):
        frames = frames.detach().cpu().numpy()
    frames = np.asarray(frames)
    s = _samples_of(frames, pixel_format, size, depth)
    n = s.shape[0]
    if n < 1:
        raise ValueError("the video has no frames")
    if hw:
        q = s.reshape(n, hw[0], hw[1], 1)
    elif frames.dtype == np.uint8:
        q = s.reshape(frames.shape)
    else:
        q = s.reshape(frames.shape).transpose(0, 2, 3, 1)
    q = q.astype(np.int64)
    return q.sum(axis=(2, 3), dtype=np.int64), q.sum(axis=(1, 3), dtype=np.int64)


def line_samples(h: int, w: int, c: int = 1) -> Tuple[int, int]:
    """(S_row, S_col), the samples a row and a column of h x w frames hold: (c * w, c * h) of packed frames of c channels, (w, h) of
    planar ones (c = 1: the Y plane)."""
    return c * w, c * h


def check_limit(limit) -> Fraction:
    """The limit as an exact fraction; refuses a non-number, a non-finite one and one outside 0 <= limit < 255."""
    if isinstance(limit, bool) or not isinstance(limit, (int, float, Fraction)):
        raise ValueError(f"crop_limit must be a number (the largest mean of a black line, on the 8-bit scale), got {limit!r}")
    if isinstance(limit, float) and not math.isfinite(limit):
        raise ValueError(f"crop_limit must be finite, got {limit!r}")
    lim = Fraction(limit)
    if not 0 <= lim < 255:
        raise ValueError(f"crop_limit must be in 0 <= limit < 255 (the 8-bit scale), got {limit!r}")
    return lim


def active_rect(row_max: Sequence[int], col_max: Sequence[int], s_row: int, s_col: int, limit=DEFAULT_LIMIT) -> Rect:
    """(y0, x0, ah, aw) of the picture, from row_max[k] = the largest sum of row k over the frames and col_max likewise (`line_sums`),
    s_row / s_col = the samples a row / a column holds.  ffmpeg cropdetect's rule in exact arithmetic: a line is black iff
    sum <= limit * S (a whole line at exactly `limit` per sample is black, one more is picture); the picture spans the first to the last
    row that is not black, and the same for the columns.  No such line, or a span below 2 x 2 (what SAVSR needs): the whole frame."""
    lim = check_limit(limit)
    if s_row < 1 or s_col < 1:
        raise ValueError(f"s_row = {s_row}, s_col = {s_col}: a line holds at least one sample")
    h, w = len(row_max), len(col_max)
    ys = [k for k, v in enumerate(row_max) if int(v) > lim * int(s_row)]
    xs = [k for k, v in enumerate(col_max) if int(v) > lim * int(s_col)]
    if not ys or not xs:
        return 0, 0, h, w
    y0, x0, ah, aw = ys[0], xs[0], ys[-1] - ys[0] + 1, xs[-1] - xs[0] + 1
    if ah < 2 or aw < 2:
        return 0, 0, h, w
    return y0, x0, ah, aw


def align_rect(rect: Rect, layout: Optional[str]) -> Rect:
    """The rect with its offsets moved outwards to the chroma block of the input layout: y0 down to a multiple of 2 for "420", x0 down
    to a multiple of 2 for "420" and "422", nothing for "444", "400" and packed frames (None).  The far edges stay where they are (odd
    sizes are first class).  Never inwards: no picture line is lost, a line of bar may stay."""
    bv, bh = block_of(layout)
    y0, x0, ah, aw = (int(v) for v in rect)
    return y0 - y0 % bv, x0 - x0 % bh, ah + y0 % bv, aw + x0 % bh


def check_rect(rect, h: Optional[int], w: Optional[int], layout: Optional[str]) -> Rect:
    """An explicit crop rect as ints: (y0, x0, ah, aw) inside the h x w frame (h = None: the size is not known yet) with ah, aw >= 2, on
    the input layout's chroma block.  An off-block rect is refused with the aligned rect it could have been; it is never moved."""
    try:
        vals = tuple(rect)
        ok = len(vals) == 4 and all(not isinstance(v, bool) and isinstance(v, (int, np.integer)) for v in vals)
    except TypeError:
        ok = False
    if not ok or isinstance(rect, (str, bytes)):
        raise ValueError(f"crop = {rect!r}: None, 'auto' or a rect (y0, x0, ah, aw) of ints")
    y0, x0, ah, aw = (int(v) for v in vals)
    if y0 < 0 or x0 < 0 or ah < 2 or aw < 2:
        raise ValueError(f"crop = {(y0, x0, ah, aw)}: a rect (y0, x0, ah, aw) has y0, x0 >= 0 and ah, aw >= 2 (SAVSR needs h, w >= 2)")
    if h is not None and (y0 + ah > h or x0 + aw > w):
        raise ValueError(f"crop = {(y0, x0, ah, aw)} does not lie inside the {h} x {w} frame")
    if align_rect((y0, x0, ah, aw), layout) != (y0, x0, ah, aw):
        raise ValueError(f"crop = {(y0, x0, ah, aw)} is off the chroma block of 4:{layout[1]}:{layout[2]} frames (offsets in multiples of "
                         f"{' x '.join(str(b) for b in block_of(layout))}); the aligned rect is {align_rect((y0, x0, ah, aw), layout)}")
    return y0, x0, ah, aw


def check_bars(bars) -> str:
    if not isinstance(bars, str) or bars not in BARS:
        raise ValueError(f"bars = {bars!r}: one of {', '.join(BARS)}")
    return bars


# ---- where the picture goes in the output ------------------------------------------------------------------------------------------------
def place(rect: Rect, h: int, w: int, scale, out_layout: Optional[str]) -> Tuple[int, int, int, int, int, int]:
    """(H_f, W_f, H_a, W_a, Y0, X0): the output sizes of the full h x w frame and of the rect (packing.get_hw), and where the upscaled
    picture's top-left corner sits in the full output.  With B the output layout's block along the axis (2 for the rows of "420" and the
    columns of "420" / "422", else 1): Y0 = B * round(y0 * sh / B) (Python round), then clamped to <= H_f - H_a and taken down to a
    multiple of B; X0 likewise.  Hence 0 <= Y0, Y0 % B == 0 and Y0 + H_a <= H_f for every scale."""
    y0, x0, ah, aw = rect
    sh, sw = float(scale[0]), float(scale[1])
    Hf, Wf = get_hw(h, w, (sh, sw))
    Ha, Wa = get_hw(ah, aw, (sh, sw))
    bv, bh = block_of(out_layout)

    def corner(o: int, s: float, b: int, room: int) -> int:
        p = min(b * round(o * s / b), room)
        return p - p % b

    return Hf, Wf, Ha, Wa, corner(y0, sh, bv, Hf - Ha), corner(x0, sw, bh, Wf - Wa)


def _planes(frames: np.ndarray, h: int, w: int, depth: int, layout: str):
    if layout == MONO:
        return [luma_plane(frames, h, w, depth, MONO)]
    return list(split_planes(frames, h, w, depth, layout))


def _join(planes, depth: int) -> np.ndarray:
    n = planes[0].shape[0]
    return np.concatenate([np.ascontiguousarray(p.astype(np.uint8 if depth == 8 else "<u2")).reshape(n, -1).view(np.uint8) for p in planes], 1)


def _plane_rect(rect: Rect, layout: str, k: int) -> Rect:
    """The rect of plane k (0 = Y) of a planar frame: the offsets divided by the plane's block, the size that of the layout's plane."""
    y0, x0, ah, aw = rect
    if k == 0:
        return rect
    bv, bh = block_of(layout)
    return (y0 // bv, x0 // bh) + chroma_hw(ah, aw, layout)


def crop_frames(frames, rect: Rect, fmt: str = "rgb", size=None, depth: int = 8) -> np.ndarray:
    """The hand crop of a video to rect = (y0, x0, ah, aw).  Packed frames (fmt "rgb", "uint8", "float"): [N, h, w, c] uint8 ->
    [N, ah, aw, c], [N, c, h, w] float -> [N, c, ah, aw].  Planar frames (fmt "i420", "i422", "i444", "y400" with size=(h, w)):
    [N, frame_bytes(h, w, depth, layout)] uint8 -> [N, frame_bytes(ah, aw, depth, layout)], every plane cropped at the rect divided by
    its block; the offsets must sit on the block (`align_rect`)."""
    if hasattr(frames, "detach"):
        frames = frames.detach().cpu().numpy()
    frames = np.asarray(frames)
    y0, x0, ah, aw = (int(v) for v in rect)
    if fmt not in SAMPLE_FORMATS:
        if frames.ndim != 4:
            raise ValueError(f"frames must be [N, h, w, c] uint8 or [N, c, h, w] float, got {frames.ndim} dimensions")
        h, w = frames.shape[1:3] if frames.dtype == np.uint8 else frames.shape[2:4]
        check_rect((y0, x0, ah, aw), h, w, None)
        return frames[:, y0:y0 + ah, x0:x0 + aw] if frames.dtype == np.uint8 else frames[:, :, y0:y0 + ah, x0:x0 + aw]
    h, w = check_pixel_format(fmt, size)
    layout, depth = layout_of(fmt), check_depth(depth)
    check_rect((y0, x0, ah, aw), h, w, layout)
    out = []
    for k, p in enumerate(_planes(frames, h, w, depth, layout)):
        py, px, ph, pw = _plane_rect((y0, x0, ah, aw), layout, k)
        out.append(p[:, py:py + ph, px:px + pw])
    return _join(out, depth)


def bars_frame(H: int, W: int, out: str, depth: int = 8, colour: str = "bt601", nch: int = 3) -> np.ndarray:
    """One full-size output frame of nominal black, the bars of `insert_frames`: packed frames ("float" [c, H, W] float32, "uint8"
    [H, W, c]) are 0; planar Y is 16 k at limited range and 0 at full range, planar chroma 128 k, k = 2^(depth - 8)."""
    if out == "float":
        return np.zeros((nch, H, W), np.float32)
    if out not in SAMPLE_FORMATS:
        return np.zeros((H, W, nch), np.uint8)
    layout, k = layout_of(out), 1 << (check_depth(depth) - 8)
    planes = [np.full((1, H, W), 0 if is_full_range(colour) else 16 * k, np.uint16)]
    if layout != MONO:
        planes += [np.full((1,) + chroma_hw(H, W, layout), 128 * k, np.uint16)] * 2
    return _join(planes, depth)[0]


def insert_frames(sr_active, placed, out: str = "float", depth: int = 8, colour: str = "bt601") -> np.ndarray:
    """The full-size result with bars: the upscaled picture `sr_active` (the out kind's frames of H_a x W_a) copied into frames of
    `bars_frame` (H_f x W_f) at (Y0, X0); placed = `place`'s six numbers.  The planes of planar frames are copied in at (Y0, X0) divided by
    each plane's block.  With an odd H_a in 4:2:0 the picture's last chroma row also covers the first bar row below it (and with an odd
    W_a the last chroma column the first bar column): that is the definition, not an accident -- the chroma sample belongs to a block
    the picture's last line lies in."""
    Hf, Wf, Ha, Wa, Y0, X0 = (int(v) for v in placed)
    if hasattr(sr_active, "detach"):
        sr_active = sr_active.detach().cpu().numpy()
    x = np.asarray(sr_active)
    n = x.shape[0]
    if out not in SAMPLE_FORMATS:
        c = x.shape[1] if out == "float" else x.shape[3]
        full = np.repeat(bars_frame(Hf, Wf, out, nch=c)[None], n, 0)
        if out == "float":
            full[:, :, Y0:Y0 + Ha, X0:X0 + Wa] = x
        else:
            full[:, Y0:Y0 + Ha, X0:X0 + Wa] = x
        return full
    layout, depth = layout_of(out), check_depth(depth)
    full = _planes(np.repeat(bars_frame(Hf, Wf, out, depth, colour)[None], n, 0), Hf, Wf, depth, layout)
    full = [np.array(p) for p in full]
    for k, p in enumerate(_planes(x, Ha, Wa, depth, layout)):
        py, px, ph, pw = _plane_rect((Y0, X0, Ha, Wa), layout, k)
        full[k][:, py:py + ph, px:px + pw] = p
    return _join(full, depth)
