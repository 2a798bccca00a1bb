"""Noise level: how strong is the noise of a video, in 8-bit code units -- the host-side specification (numpy, integers only, no GPU
needed).  `denoise="ata"` and `spatial_denoise="nlm"` rest on the caller knowing a strength; a tensor, a PNG folder and a Y4M stream
carry no noise figure.  This module measures one from the content.  The kernels of csrc/noise.hip equal `noise_stats_matrix` bit for
bit; the decision is host work in exact rational arithmetic.

`noise_stats_matrix(m, depth, interlaced)` -> int64 [256, 2].  Samples are v = min(m, 2^d - 1) at their own depth (not on the 8-bit
scale: a 10-bit source keeps two fractional bits of sigma).  interlaced=True takes each field (rows 0::2, rows 1::2) as a plane of its
own, both adding into the one table.  Per plane of R x C:
    h[y][x] = v[y][x - 1] - 2 v[y][x] + v[y][x + 1]
    L[y][x] = |h[y - 1][x] - 2 h[y][x] + h[y + 1][x]|          for 1 <= y <= R - 2, 1 <= x <= C - 2
-- the 3 x 3 mask [1 -2 1]^T (x) [1 -2 1], which annihilates planes and ramps and has standard deviation 6 sigma on white noise.  Cell
(i, j), i < (R - 2) // 8, j < (C - 2) // 8, holds the 64 values L[8i + 1 .. 8i + 8][8j + 1 .. 8j + 8]; values outside a full cell
belong to no cell, and a plane below 10 x 10 has none.  A cell is FLAT iff one of its 8 row sums or one of its 8 column sums of L is 0
(constant areas, and cells that straddle the edge of a bar, which would read half the noise): table[255][0] += 1 and nothing else.  Any
other cell has S = (sum of L) >> (d - 8) and b = min(S >> 4, 254): table[b][0] += 1, table[b][1] += S.  The sums are kept, so the bin
width costs no accuracy.  sum of L <= 64 * 16 * 4095 < 2^32.

`noise_stats_frames` -> [N, 2, 256, 2]: class 0 is the Y plane, or every channel of packed [N, h, w, c] uint8 frames as a plane of its
own; class 1 is Cb + Cr, zeros where there is none.

`verdict_from_stats(table[2, 256, 2], quantile, min_cells, floor)`, the table summed over the frames, per class: N = the cells of the
rows below 255; N < min_cells: undetermined.  k = ceil(N * quantile); walking the rows upwards, take t_b = min(left, count_b) cells from
each at the row's mean: T = sum of t_b * sum_b / count_b; sigma = T / (245 k), a Fraction in 8-bit code units.  245 = rint(64 * 6 *
sqrt(2 / pi) * 4 / 5): 64 samples of a cell, E|L| = 6 sigma sqrt(2 / pi) for white Gaussian noise, and 5 / 4 the ratio of the mean cell
to the mean of the lowest quarter of the cells -- measured on this rule, not derived.

`NoiseVerdict.spatial_kwargs(gain=3/2)`: {} where sigma is unknown or below `floor`; else spatial_strength = min(32, floor(16 gain
sigma + 1/2) / 16) (identical patches under noise sigma differ by a mean square of 2 sigma^2, which h = 1.5 sigma weighs about 1 / e;
sigma = 2 gives the default 3.0), and spatial_chroma_strength the same map of max(chroma sigma, floor) where that is known.
`NoiseVerdict.denoise_kwargs(gain=3)`: {} likewise; else A = min(255, ceil(gain sigma)), B = min(255, 2 A + 1), denoise_strength =
(A, B) (sigma = 4/3 gives the default (4, 9)); denoise_chroma_strength the same map of a known chroma sigma, (0, 0) -- the rule's
identity -- below `floor`.

The measure, the constants (the lowest quarter, 245, min_cells 64, floor 1/2) and the two gains are this project's own.  They separate
synthetic pictures (128 + 60 sin(x / 11) cos(y / 13) plus sigma noise, with and without bars; tests/test_noise.py holds the set) and
are NOT validated on footage or on trained weights.  Limits: one figure per video; a white-noise model, so coarse film grain and the
noise of subsampled chroma read low; texture over more than three quarters of the frame reads high; clipped shadows and highlights read
low.
"""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction
from typing import Dict, Optional, Tuple

import numpy as np

from .deblock import _is_int, _planes
from .frames import check_pixel_format, layout_of
from .yuv import check_depth, frame_bytes, layout_name

ROWS = 256                                # of a table: 255 bins of S >> 4 and the flat cells' row
FLAT = 255
CELL = 8
NORM = 245                                # rint(64 * 6 * sqrt(2 / pi) * 4 / 5)
DEFAULT_QUANTILE = Fraction(1, 4)         # parameters of this project's own: nothing is validated on footage
DEFAULT_MIN_CELLS = 64
DEFAULT_FLOOR = Fraction(1, 2)
DEFAULT_SPATIAL_GAIN = Fraction(3, 2)
DEFAULT_DENOISE_GAIN = Fraction(3)
NOISE_FLAGS = ("auto",)


def is_auto(strength) -> bool:
    """Whether a strength argument is the flag "auto"."""
    return isinstance(strength, str) and strength in NOISE_FLAGS


def _fraction(value, what: str, why: str) -> Fraction:
    try:
        if isinstance(value, bool):
            raise TypeError
        return Fraction(value)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{what} = {value!r}: {why}") from None


def check_quantile(quantile, what: str = "quantile") -> Fraction:
    """The share of the binned cells, from the quietest upwards, whose mean is read: 0 < q <= 1, kept as an exact fraction."""
    why = "a number with 0 < q <= 1 (the share of the cells, from the quietest upwards, whose mean is read)"
    q = _fraction(quantile, what, why)
    if not 0 < q <= 1:
        raise ValueError(f"{what} = {quantile!r}: {why}")
    return q


def check_min_cells(min_cells, what: str = "min_cells") -> int:
    """The fewest binned cells a class is decided on: an int >= 1."""
    if not _is_int(min_cells) or min_cells < 1:
        raise ValueError(f"{what} = {min_cells!r}: an int >= 1 (the fewest cells that are not flat a noise level is read from)")
    return int(min_cells)


def check_floor(floor, what: str = "floor") -> Fraction:
    """The sigma below which no noise is reported: a finite number >= 0 in 8-bit code units, kept as an exact fraction."""
    why = "a finite number >= 0 (the sigma, in 8-bit code units, below which there is no noise to remove)"
    f = _fraction(floor, what, why)
    if f < 0:
        raise ValueError(f"{what} = {floor!r}: {why}")
    return f


def check_gain(gain, what: str = "gain") -> Fraction:
    """Strength per sigma: a finite number above 0, kept as an exact fraction."""
    why = "a finite number above 0 (the strength per sigma)"
    g = _fraction(gain, what, why)
    if g <= 0:
        raise ValueError(f"{what} = {gain!r}: {why}")
    return g


def _plane_stats(v: np.ndarray, shift: int, out: np.ndarray) -> None:
    R, C = v.shape
    ny, nx = (R - 2) // CELL, (C - 2) // CELL
    if R < CELL + 2 or C < CELL + 2:
        return
    h = v[:, :-2] - 2 * v[:, 1:-1] + v[:, 2:]
    L = np.abs(h[:-2] - 2 * h[1:-1] + h[2:])[:CELL * ny, :CELL * nx].reshape(ny, CELL, nx, CELL)
    flat = (L.sum(3) == 0).any(1) | (L.sum(1) == 0).any(2)
    S = L.sum((1, 3)) >> shift
    out[FLAT, 0] += int(flat.sum())
    S = S[~flat]
    b = np.minimum(S >> 4, FLAT - 1)
    np.add.at(out[:, 0], b, 1)
    np.add.at(out[:, 1], b, S)


def noise_stats_matrix(m, depth: int = 8, interlaced: bool = False) -> np.ndarray:
    """[R, C] integer samples -> int64 [256, 2]: per row b < 255 the count and the sum of S of the cells with S >> 4 = b (254: and
    above), row 255 the count of the flat cells (the module's docstring); interlaced: field by field, both into the one table."""
    m = np.asarray(m)
    if m.ndim != 2 or m.dtype.kind not in "iu":
        raise ValueError(f"the matrix must be [R, C] integers, got {m.dtype} {tuple(m.shape)}")
    if m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError(f"a matrix of {m.shape[0]} x {m.shape[1]}: R >= 1 and C >= 1")
    if depth not in (8, 10, 12):
        raise ValueError(f"depth = {depth!r}: 8, 10 or 12")
    v = np.minimum(m.astype(np.int64), (1 << depth) - 1)
    out = np.zeros((ROWS, 2), np.int64)
    for f in ((v[0::2], v[1::2]) if interlaced else (v,)):
        _plane_stats(f, depth - 8, out)
    return out


def noise_stats_frames(frames, pixel_format: str = "rgb", size=None, depth: int = 8, interlaced: bool = False) -> np.ndarray:
    """N frames -> int64 [N, 2, 256, 2]: `noise_stats_matrix` per frame and class.  Class 0: the Y plane of planar frames (pixel_format
    "i420", "i422", "i444", "y400" with size=(h, w); [N, frame_bytes] uint8, little-endian 16-bit words at depth 10 / 12), or every channel
    of [N, h, w, c] uint8 frames as a plane of its own; class 1: Cb + Cr, zeros where there is none.  Float frames are refused."""
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
        out = np.zeros((frames.shape[0], 2, ROWS, 2), np.int64)
        for i, pl in enumerate(_planes(frames, h, w, depth, layout)):
            for t in range(frames.shape[0]):
                out[t, min(i, 1)] += noise_stats_matrix(pl[t], depth, interlaced)
        return out
    if depth != 8:
        raise ValueError(f"depth = {depth} goes with pixel_format = 'i420', 'i422', 'i444' or 'y400': packed frames are 8-bit")
    if frames.dtype.kind == "f":
        raise ValueError("float frames have no integer samples to measure noise in: give [N, h, w, c] uint8 or planar frames (quantise first)")
    if frames.dtype != np.uint8 or frames.ndim != 4:
        raise ValueError(f"frames must be [N, h, w, c] uint8, got {frames.dtype} {tuple(frames.shape)}")
    out = np.zeros((frames.shape[0], 2, ROWS, 2), np.int64)
    for t in range(frames.shape[0]):
        for ch in range(frames.shape[3]):
            out[t, 0] += noise_stats_matrix(frames[t, :, :, ch], 8, interlaced)
    return out


def _sixteenths(x: Fraction) -> Fraction:
    """x rounded half up to a multiple of 1/16."""
    return Fraction((16 * x + Fraction(1, 2)).__floor__(), 16)


@dataclass(frozen=True)
class NoiseVerdict:
    """sigma: the noise level of class 0 (the Y plane, or all channels of packed frames) as a Fraction in 8-bit code units, None where
    fewer than min_cells cells were not flat; chroma_sigma: that of Cb + Cr, None where there are no chroma planes or too few cells;
    cells, flat: per class the binned and the flat cells; table: the [2, 256, 2] sums the decision read; floor: the sigma below which the
    maps report no noise."""
    sigma: Optional[Fraction]
    chroma_sigma: Optional[Fraction]
    cells: Tuple[int, int]
    flat: Tuple[int, int]
    table: np.ndarray
    floor: Fraction = DEFAULT_FLOOR

    def _noisy(self) -> bool:
        return self.sigma is not None and self.sigma >= self.floor

    def spatial_kwargs(self, gain=DEFAULT_SPATIAL_GAIN) -> Dict[str, object]:
        """The explicit arguments of upscale_video (beside spatial_denoise=) that say the same; {} where no noise was found (the call
        then runs without the stage)."""
        gain = check_gain(gain)
        if not self._noisy():
            return {}
        to_h = lambda s: float(min(Fraction(32), _sixteenths(gain * s)))          # noqa: E731
        out: Dict[str, object] = dict(spatial_strength=to_h(self.sigma))
        if self.chroma_sigma is not None:
            out.update(spatial_chroma_strength=to_h(max(self.chroma_sigma, self.floor)))
        return out

    def denoise_kwargs(self, gain=DEFAULT_DENOISE_GAIN) -> Dict[str, object]:
        """The explicit arguments of upscale_video (beside denoise=) that say the same; {} where no noise was found.  Chroma planes
        whose noise lies below the floor are left alone: (0, 0) is the rule's identity."""
        gain = check_gain(gain)
        if not self._noisy():
            return {}

        def to_ab(s: Fraction):
            a = min(255, (gain * s).__ceil__())
            return a, min(255, 2 * a + 1)
        out: Dict[str, object] = dict(denoise_strength=to_ab(self.sigma))
        if self.chroma_sigma is not None:
            out.update(denoise_chroma_strength=to_ab(self.chroma_sigma) if self.chroma_sigma >= self.floor else (0, 0))
        return out

    def as_json(self) -> dict:
        """What --noise-out writes of one measuring point."""
        frac = lambda s: None if s is None else dict(fraction=[s.numerator, s.denominator], value=float(s))          # noqa: E731
        return dict(sigma=frac(self.sigma), chroma_sigma=frac(self.chroma_sigma), cells=list(self.cells), flat=list(self.flat),
                    floor=float(self.floor), table=np.asarray(self.table).tolist())


def _class_sigma(table: np.ndarray, quantile: Fraction, min_cells: int) -> Tuple[Optional[Fraction], int]:
    counts = [int(c) for c in table[:FLAT, 0]]
    N = sum(counts)
    if N < min_cells:
        return None, N
    k = (N * quantile).__ceil__()
    left, T = k, Fraction(0)
    for b, c in enumerate(counts):
        if not left:
            break
        t = min(left, c)
        if t:
            T += Fraction(t * int(table[b, 1]), c)
            left -= t
    return T / (NORM * k), N


def verdict_from_stats(table, quantile=DEFAULT_QUANTILE, min_cells: int = DEFAULT_MIN_CELLS, floor=DEFAULT_FLOOR) -> NoiseVerdict:
    """table: int [2, 256, 2], summed over the frames -> the NoiseVerdict (the module's docstring has the rule).  The defaults are this
    project's own and are not validated on footage."""
    quantile, min_cells, floor = check_quantile(quantile), check_min_cells(min_cells), check_floor(floor)
    table = np.asarray(table)
    if table.shape != (2, ROWS, 2) or table.dtype.kind not in "iu":
        raise ValueError(f"table is [2, {ROWS}, 2] integers (summed over the frames), got {table.dtype} {tuple(table.shape)}")
    if np.any(table < 0) or np.any(table[:, FLAT, 1] != 0):
        raise ValueError(f"table holds counts and sums >= 0, and no sum in row {FLAT} (the flat cells)")
    (s0, n0), (s1, n1) = (_class_sigma(table[k], quantile, min_cells) for k in (0, 1))
    return NoiseVerdict(s0, s1, (n0, n1), (int(table[0, FLAT, 0]), int(table[1, FLAT, 0])), table.astype(np.int64), floor)


def estimate_noise_frames(frames, pixel_format: str = "rgb", size=None, depth: int = 8, interlaced: bool = False, quantile=DEFAULT_QUANTILE,
                          min_cells: int = DEFAULT_MIN_CELLS, floor=DEFAULT_FLOOR) -> NoiseVerdict:
    """`verdict_from_stats` on `noise_stats_frames` summed over the frames: what savsr_amd.estimate_noise computes on the GPU."""
    return verdict_from_stats(noise_stats_frames(frames, pixel_format, size, depth, interlaced).sum(0), quantile, min_cells, floor)
