"""Ordered dither for the integer outputs of the sequence path: the specification of the `_d` quantiser entries
(savsr_video_quantize_u8_d / _yuvs_d / _luma_d; csrc/dither.hpp is the twin) and of `dither=` on upscale_video, VideoUpscaler and the CLI.
numpy only.

Where a quantiser computes rint(t) it computes floor(t + theta(y, x)) with `dither="ordered"`: t the float32 value in output code units
(clamp01(v) * 255 for packed RGB, row * k for Y / Cb / Cr, clamp01(v) * 255 k for luma), theta a position-dependent threshold from a
16 x 16 Bayer matrix.  The sum is ONE float32 addition (round to nearest even), not contracted with the multiply in front of it; floor
follows, then exactly the clips that follow rint without a dither (0 .. 255 for the full-range colour spaces, none for limited range).

  B2 = [[0, 2], [3, 1]];  B2n[y][x] = 4 Bn[y mod n][x mod n] + B2[y div n][x div n];  B = B16, every value 0 .. 255 once.
  Closed form, 0 <= x, y < 16:  B[y][x] = sum over b = 0 .. 3 of 4^(3 - b) (2 (((x ^ y) >> b) & 1) + ((y >> b) & 1)).
  theta(y, x) = float32((B[y & 15][x & 15] + 0.5) / 256): exact in float32, inside (0, 1).

(y, x) are the sample's coordinates in its own plane of the tensor the quantiser is handed: pixel coordinates for Y and packed RGB,
chroma-sample coordinates for Cb / Cr; the channels of a packed pixel share one threshold (the dither is grey).  The pattern does not
depend on the frame index: any chunking of a video gives the same bytes, and a static pattern costs an encoder nothing.

What follows from the rule (tests/test_dither.py checks each):
  * an integer t is written as it is (theta < 1), so exact codes pass unchanged;
  * limited range stays inside its nominal range without a clip;
  * a constant t = i + j / 256 gives every aligned 16 x 16 block the sum 256 i + j exactly: the block mean carries 8 more bits.

Limits: one pattern (no blue noise, no error diffusion: a serial dependency per row is not for the GPU path); static in time; the
luma-only path's Cb / Cr (resampled samples, not network output) keep rint; nothing is validated on real footage or trained weights.
"""
from __future__ import annotations

from functools import lru_cache
from typing import Optional

import numpy as np

# The dithers of `dither=`; the id of the C ABI (SAVSR_DITHER_*) is the position plus one, 0 (None) = round to nearest.
DITHERS = ("ordered",)
N = 16          # the matrix's side


def check_dither(dither, what: str = "dither") -> Optional[str]:
    """None or one of DITHERS, returned as it is; refuses anything else, naming the list."""
    if dither is None:
        return None
    if not isinstance(dither, str) or dither not in DITHERS:
        raise ValueError(f"{what} = {dither!r}: None or one of {', '.join(DITHERS)}")
    return dither


def dither_id(dither) -> int:
    """The C-ABI id of a dither: 0 for None, the position in DITHERS plus one otherwise."""
    return 0 if check_dither(dither) is None else DITHERS.index(dither) + 1


def bayer(n: int = N) -> np.ndarray:
    """The n x n index matrix (n a power of two >= 2) by the recursion, int64: every value 0 .. n * n - 1 once."""
    if not isinstance(n, (int, np.integer)) or isinstance(n, bool) or n < 2 or n & (n - 1):
        raise ValueError(f"bayer({n!r}): a power of two >= 2")
    b2 = np.array([[0, 2], [3, 1]], np.int64)
    if n == 2:
        return b2
    h = n // 2
    return 4 * np.tile(bayer(h), (2, 2)) + np.repeat(np.repeat(b2, h, 0), h, 1)


@lru_cache(maxsize=None)
def _theta() -> np.ndarray:
    t = ((bayer(N).astype(np.float64) + 0.5) / 256.0).astype(np.float32)
    t.setflags(write=False)
    return t


def thresholds() -> np.ndarray:
    """theta as float32 [16, 16] (read-only): (B + 0.5) / 256, exact."""
    return _theta()


def threshold_field(h: int, w: int) -> np.ndarray:
    """theta(y & 15, x & 15) over an h x w plane, float32 [h, w]."""
    return _theta()[np.ix_(np.arange(h) & (N - 1), np.arange(w) & (N - 1))]


def dither_floor(t: np.ndarray) -> np.ndarray:
    """floor(t + theta(y, x)) of float32 [..., H, W] in code units, as float32: one float32 addition, then floor."""
    t = np.asarray(t)
    if t.dtype != np.float32 or t.ndim < 2:
        raise ValueError(f"values in code units are [..., H, W] float32, got {t.dtype} {tuple(t.shape)}")
    return np.floor(t + threshold_field(t.shape[-2], t.shape[-1]))


def quantise(t: np.ndarray, dither=None) -> np.ndarray:
    """What a quantiser makes of float32 [..., H, W] in code units, as float32: rint (half to even) or, dithered, `dither_floor`."""
    return np.rint(t) if check_dither(dither) is None else dither_floor(t)


def rgb_to_u8(x: np.ndarray, dither=None) -> np.ndarray:
    """Packed frames of float ones, [N, c, H, W] float32 -> [N, H, W, c] uint8 (savsr_video_quantize_u8 / _u8_d): clamp to [0, 1]
    (fmax / fmin: a NaN becomes 0), x 255.0f, then rint or the dither's rule at the pixel's (y, x), the same for every channel."""
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim != 4:
        raise ValueError(f"float frames are [N, c, H, W] float32, got {x.dtype} {tuple(x.shape)}")
    t = np.fmin(np.fmax(x, np.float32(0)), np.float32(1)) * np.float32(255)
    return np.ascontiguousarray(quantise(t, dither).astype(np.uint8).transpose(0, 2, 3, 1))
