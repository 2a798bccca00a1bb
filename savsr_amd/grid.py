"""Block-grid detection: which block size and which origin does the blocking of a video have, if any -- the host-side specification
(numpy, integers only, no GPU needed).  `deblock=` rests on the caller knowing the grid; a tensor or a PNG folder carries neither the
codec's block size nor the crop that moved the grid away from the frame's origin.  This module finds both from the content.  The kernels
of csrc/grid.hip equal `grid_stats_matrix` bit for bit; the decision is host work in exact rational arithmetic.

`grid_stats_matrix(m, depth, interlaced, cap)` -> int64 [2, 16].  Samples are read as min(s, 2^d - 1) >> (d - 8), the detectors' 8-bit
scale.  Along a line v of length L consider every boundary x with 2 <= x <= L - 2 and
    s = |v[x] - v[x - 1]|,   l = |v[x - 1] - v[x - 2]|,   r = |v[x + 1] - v[x]|:
the boundary is a hit iff s > l + r and s <= cap -- a step larger than the slopes on both of its sides, and small enough not to be
picture.  out[0][x mod 16] counts the hits along the rows (x in pixels), out[1][y mod 16] those along the columns.  interlaced=True takes
each field (rows 0::2, rows 1::2) as a plane of its own for the columns, y being the field row, and the two fields add into the same 16
cells; the rows' counts are what they are without it.  Lines shorter than 4 have no boundary.

`grid_pairs(rows, cols, interlaced)` -> int64 [2, 16]: how many boundaries each cell of `grid_stats_matrix` counts over (host work: the
GPU does not count them).  `grid_stats_frames` -> [N, 2, 2, 16]: class 0 is the Y plane, or every channel of packed frames as a plane of
its own; class 1 is Cb + Cr, zeros where there is none.  `frame_pairs` is its `grid_pairs`.

`verdict_from_stats(table, pairs, interlaced, ratio, min_count)`, table and pairs [2, 2, 16] summed over the frames, per class and
direction: rate[p] = cnt[p] / pairs[p]; the median is the mean of the 8th and the 9th of the 16 sorted rates; p is a peak iff
cnt[p] >= min_count and rate[p] >= ratio * median.  The peak set S reads: block 16 at q iff S = {q}; block 8 at q iff S = {q, q + 8};
block 4 at q iff S = {q, q + 4, q + 8, q + 12}; anything else, and a direction with an empty cell in `pairs`, is no answer.  Progressive:
a class has the grid (b, (oy, ox)) iff both directions answer with the same b (the rows give ox, the columns oy).  Interlaced: the rows
must answer b in {8, 16} and the columns, counted in field rows, b / 2 at q: oy = 2 q; at b = 4 the fields' blocks have two rows, the
deblocker has no pass Y there, the columns are not consulted and oy = 0.  The verdict's block and origin are class 0's; chroma_origin
is class 1's origin when its block equals class 0's, else None.

The measure, the rule and its defaults (cap 32, ratio 3/2, min_count 64) are this project's own.  They separate synthetic pictures
(128 + 60 sin(x / 11) cos(y / 13) plus an offset in -a .. a per block plus sigma noise at 288 x 352; tests/test_grid.py holds the set) and
are NOT validated on footage.  Limits: one grid per video; grids of scaled video and block sizes other than 4, 8 and 16 are not found;
block 4 on noise-free material is missed (the median is near zero there and stray cells pass min_count); small planes carry too few
boundaries; periodic picture content of period 4, 8 or 16 can fake a grid.
"""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction
from typing import Dict, Optional, Tuple

import numpy as np

from .deblock import _is_int, _planes
from .frames import check_pixel_format, layout_of
from .yuv import MONO, check_depth, chroma_hw, frame_bytes, layout_name

CELLS = 16
DEFAULT_CAP = 32                          # parameters of this project's own: nothing is validated on footage
DEFAULT_RATIO = Fraction(3, 2)
DEFAULT_MIN_COUNT = 64
GRID_FLAGS = ("auto",)


def check_cap(cap, what: str = "cap") -> int:
    """The largest step that counts as a block edge: an int in 0 .. 255, in 8-bit code units at every depth."""
    if not _is_int(cap) or not 0 <= cap <= 255:
        raise ValueError(f"{what} = {cap!r}: an int in 0 .. 255 (the largest step, in 8-bit code units, that counts as a block edge)")
    return int(cap)


def check_ratio(ratio, what: str = "ratio") -> Fraction:
    """How far above the median rate a peak stands: a finite number above 1, kept as an exact fraction."""
    try:
        if isinstance(ratio, bool):
            raise TypeError
        r = Fraction(ratio)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{what} = {ratio!r}: a finite number above 1 (a peak's rate over the median rate)") from None
    if r <= 1:
        raise ValueError(f"{what} = {ratio!r}: a finite number above 1 (a peak's rate over the median rate)")
    return r


def check_min_count(min_count, what: str = "min_count") -> int:
    """The fewest hits a peak cell holds: an int >= 1."""
    if not _is_int(min_count) or min_count < 1:
        raise ValueError(f"{what} = {min_count!r}: an int >= 1 (the fewest hits a peak cell holds)")
    return int(min_count)


def _lines(v: np.ndarray, cap: int) -> np.ndarray:
    """int64 [16]: the hits along the last axis of v (int64 [lines, L]) by x mod 16."""
    out = np.zeros(CELLS, np.int64)
    L = v.shape[1]
    if L < 4 or not v.shape[0]:
        return out
    d = np.abs(np.diff(v, axis=1))          # d[:, i] = |v[i + 1] - v[i]|
    x = np.arange(2, L - 1)
    s, l, r = d[:, x - 1], d[:, x - 2], d[:, x]
    hit = (s > l + r) & (s <= cap)
    np.add.at(out, x % CELLS, hit.sum(0))
    return out


def grid_stats_matrix(m, depth: int = 8, interlaced: bool = False, cap: int = DEFAULT_CAP) -> np.ndarray:
    """[R, C] integer samples -> int64 [2, 16]: the hits along the rows by x mod 16 and along the columns by y mod 16 (the module's
    docstring); interlaced: the columns field by field, y the field row."""
    cap = check_cap(cap)
    m = np.asarray(m)
    if m.ndim != 2 or m.dtype.kind not in "iu":
        raise ValueError(f"the matrix must be [R, C] integers, got {m.dtype} {tuple(m.shape)}")
    if m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError(f"a matrix of {m.shape[0]} x {m.shape[1]}: R >= 1 and C >= 1")
    if depth not in (8, 10, 12):
        raise ValueError(f"depth = {depth!r}: 8, 10 or 12")
    v = np.minimum(m.astype(np.int64), (1 << depth) - 1) >> (depth - 8)
    out = np.zeros((2, CELLS), np.int64)
    out[0] = _lines(v, cap)
    for f in ((v[0::2], v[1::2]) if interlaced else (v,)):
        out[1] += _lines(f.T, cap)
    return out


def _cells(L: int, lines: int) -> np.ndarray:
    out = np.zeros(CELLS, np.int64)
    if L >= 4:
        np.add.at(out, np.arange(2, L - 1) % CELLS, lines)
    return out


def grid_pairs(rows: int, cols: int, interlaced: bool = False) -> np.ndarray:
    """int64 [2, 16]: the boundaries behind each cell of `grid_stats_matrix` on a rows x cols matrix."""
    out = np.zeros((2, CELLS), np.int64)
    out[0] = _cells(cols, rows)
    for n in (((rows + 1) // 2, rows // 2) if interlaced else (rows,)):
        out[1] += _cells(n, cols)
    return out


def _shapes(frames_shape, pixel_format: str, size, depth: int):
    """((rows, cols, planes) of class 0, of class 1 or None) of frames of this kind."""
    hw = check_pixel_format(pixel_format, size)
    if not hw:
        if len(frames_shape) != 4:
            raise ValueError(f"frames must be [N, h, w, c] uint8, got {tuple(frames_shape)}")
        return (int(frames_shape[1]), int(frames_shape[2]), int(frames_shape[3])), None
    h, w = hw
    layout = layout_of(pixel_format)
    if layout == MONO:
        return (h, w, 1), None
    ch, cw = chroma_hw(h, w, layout)
    return (h, w, 1), (ch, cw, 2)


def frame_pairs(frames_shape, pixel_format: str = "rgb", size=None, depth: int = 8, interlaced: bool = False) -> np.ndarray:
    """int64 [2, 2, 16]: `grid_pairs` of one frame by class, the planes of a class added."""
    out = np.zeros((2, 2, CELLS), np.int64)
    for k, shape in enumerate(_shapes(frames_shape, pixel_format, size, depth)):
        if shape:
            out[k] = shape[2] * grid_pairs(shape[0], shape[1], interlaced)
    return out


def grid_stats_frames(frames, pixel_format: str = "rgb", size=None, depth: int = 8, interlaced: bool = False, cap: int = DEFAULT_CAP) -> np.ndarray:
    """N frames -> int64 [N, 2, 2, 16]: `grid_stats_matrix` per frame and class.  Class 0: the Y plane of planar frames (pixel_format
    "i420", "i422", "i444", "y400" with size=(h, w); [N, frame_bytes] uint8, little-endian 16-bit words at depth 10 / 12), or every channel
    of [N, h, w, c] uint8 frames as a plane of its own; class 1: Cb + Cr, zeros where there is none.  Float frames are refused."""
    cap = check_cap(cap)
    hw = check_pixel_format(pixel_format, size)
    if hasattr(frames, "detach"):
        frames = frames.detach().cpu().numpy()
    frames = np.asarray(frames)
    if hw:
        h, w = hw
        layout, depth = layout_of(pixel_format), check_depth(depth)
        fb = frame_bytes(h, w, depth, layout)
        if frames.dtype != np.uint8 or frames.ndim != 2 or frames.shape[1] != fb:
            raise ValueError(f"{'' if depth == 8 else f'{depth}-bit '}{layout_name(layout)} frames of {h} x {w} are [N, {fb}] uint8, "
                             f"got {frames.dtype} {tuple(frames.shape)}")
        out = np.zeros((frames.shape[0], 2, 2, CELLS), np.int64)
        for i, pl in enumerate(_planes(frames, h, w, depth, layout)):
            for t in range(frames.shape[0]):
                out[t, min(i, 1)] += grid_stats_matrix(pl[t], depth, interlaced, cap)
        return out
    if depth != 8:
        raise ValueError(f"depth = {depth} goes with pixel_format = 'i420', 'i422', 'i444' or 'y400': packed frames are 8-bit")
    if frames.dtype.kind == "f":
        raise ValueError("float frames have no integer samples to find a grid in: give [N, h, w, c] uint8 or planar frames (quantise first)")
    if frames.dtype != np.uint8 or frames.ndim != 4:
        raise ValueError(f"frames must be [N, h, w, c] uint8, got {frames.dtype} {tuple(frames.shape)}")
    out = np.zeros((frames.shape[0], 2, 2, CELLS), np.int64)
    for t in range(frames.shape[0]):
        for ch in range(frames.shape[3]):
            out[t, 0] += grid_stats_matrix(frames[t, :, :, ch], 8, interlaced, cap)
    return out


@dataclass(frozen=True)
class GridVerdict:
    """block: 4, 8, 16 or None (no grid); origin = (oy, ox) of class 0; chroma_origin: class 1's where it has a grid of the same block,
    else None; table: the [2, 2, 16] counts the decision read; peaks: per (class, direction) the sorted peak cells; chroma: whether
    the frames have a chroma class at all."""
    block: Optional[int]
    origin: Optional[Tuple[int, int]]
    chroma_origin: Optional[Tuple[int, int]]
    table: np.ndarray
    peaks: Tuple[Tuple[Tuple[int, ...], Tuple[int, ...]], Tuple[Tuple[int, ...], Tuple[int, ...]]]
    chroma: bool = False

    def kwargs(self) -> Dict[str, object]:
        """The explicit arguments of upscale_video / VideoUpscaler (beside deblock=) that say the same; {} where there is no grid (the
        call then runs with deblock=None).  Frames with chroma planes whose grid was not found at the luma's block leave them alone:
        the chroma threshold a = 0 is the rule's identity."""
        if self.block is None:
            return {}
        out: Dict[str, object] = dict(deblock_block=self.block, deblock_origin=self.origin)
        if self.chroma:
            if self.chroma_origin is None:
                out.update(deblock_chroma_origin=(0, 0), deblock_chroma_strength=(0, 0))
            else:
                out.update(deblock_chroma_origin=self.chroma_origin)
        return out

    def as_json(self) -> dict:
        """What --grid-out writes."""
        return dict(block=self.block, origin=None if self.origin is None else list(self.origin),
                    chroma_origin=None if self.chroma_origin is None else list(self.chroma_origin),
                    table=np.asarray(self.table).tolist(), peaks=[[list(d) for d in c] for c in self.peaks])


def _direction(cnt, pairs, ratio: Fraction, min_count: int):
    """((block, q) or None, the sorted peak cells) of one class and direction."""
    if any(int(p) < 1 for p in pairs):
        return None, ()
    rate = [Fraction(int(c), int(p)) for c, p in zip(cnt, pairs)]
    srt = sorted(rate)
    median = (srt[7] + srt[8]) / 2
    S = tuple(p for p in range(CELLS) if int(cnt[p]) >= min_count and rate[p] >= ratio * median)
    for block in (16, 8, 4):
        if len(S) == CELLS // block and S == tuple(range(S[0], CELLS, block)) and S[0] < block:
            return (block, S[0]), S
    return None, S


def _class_grid(table, pairs, interlaced: bool, ratio: Fraction, min_count: int):
    """((block, (oy, ox)) or None, (the rows' peaks, the columns' peaks)) of one class."""
    (ax, sx), (ay, sy) = (_direction(table[d], pairs[d], ratio, min_count) for d in (0, 1))
    if ax is None:
        return None, (sx, sy)
    if not interlaced:
        return ((ax[0], (ay[1], ax[1])) if ay is not None and ay[0] == ax[0] else None), (sx, sy)
    if ax[0] == 4:
        return (4, (0, ax[1])), (sx, sy)
    return ((ax[0], (2 * ay[1], ax[1])) if ay is not None and 2 * ay[0] == ax[0] else None), (sx, sy)


def verdict_from_stats(table, pairs, interlaced: bool = False, ratio=DEFAULT_RATIO, min_count: int = DEFAULT_MIN_COUNT) -> GridVerdict:
    """table, pairs: int [2, 2, 16], summed over the frames -> the GridVerdict (the module's docstring has the rule).  The defaults are
    this project's own and are not validated on footage."""
    ratio, min_count = check_ratio(ratio), check_min_count(min_count)
    table, pairs = np.asarray(table), np.asarray(pairs)
    if table.shape != (2, 2, CELLS) or pairs.shape != (2, 2, CELLS) or table.dtype.kind not in "iu" or pairs.dtype.kind not in "iu":
        raise ValueError(f"table and pairs are [2, 2, {CELLS}] integers (summed over the frames), got {table.dtype} {tuple(table.shape)} and "
                         f"{pairs.dtype} {tuple(pairs.shape)}")
    (luma, lp), (chroma, cp) = (_class_grid(table[k], pairs[k], bool(interlaced), ratio, min_count) for k in (0, 1))
    has_chroma = bool(np.any(pairs[1] > 0))
    if luma is None:
        return GridVerdict(None, None, None, table.astype(np.int64), (lp, cp), has_chroma)
    co = chroma[1] if chroma is not None and chroma[0] == luma[0] else None
    return GridVerdict(luma[0], luma[1], co, table.astype(np.int64), (lp, cp), has_chroma)


def detect_grid_frames(frames, pixel_format: str = "rgb", size=None, depth: int = 8, interlaced: bool = False, ratio=DEFAULT_RATIO,
                       min_count: int = DEFAULT_MIN_COUNT, cap: int = DEFAULT_CAP) -> GridVerdict:
    """`verdict_from_stats` on `grid_stats_frames` summed over the frames: what savsr_amd.detect_grid computes on the GPU."""
    stats = grid_stats_frames(frames, pixel_format, size, depth, interlaced, cap)
    pairs = stats.shape[0] * frame_pairs(np.asarray(frames).shape if not hasattr(frames, "shape") else tuple(frames.shape), pixel_format, size, depth,
                                         interlaced)
    return verdict_from_stats(stats.sum(0), pairs, interlaced, ratio, min_count)
