"""Shared by tests/test_deblock.py, tests/test_gpu_deblock.py and tools/check_deblock_host.py: the generator of planes on which the
deblocking rule (savsr_amd/deblock.py) takes every branch, and the shapes the kernels are run at.

`case_plane`: a smooth pattern (128 + 40 sin(x / 9) cos(y / 7)) with sigma = 1 noise and an offset per `block` x `block` block drawn from
-20 .. 20, in 8-bit units scaled to the depth, so that neighbouring blocks differ by up to 40 codes: edges whose step is below the
default A = 25 are filtered, those above it are refused by A.  The right third carries sigma = 10 noise, so that steps beside an edge
reach the default Bt = 13 while the step across it stays below A: refused by Bt.  Where the plane has room, rows 1 and 2 are planted with
`.. top top top-8 | top top top ..` and `.. 0 0 8 | 0 0 0 ..` across the first vertical edge: P1 += t(8) leaves the range there and the
clamp fires at either end (tests/test_deblock.py checks the four counts at the defaults).  `above=True` also sets every (2 y, 5 x)
sample of a 16-bit plane above 2^depth - 1, where the rule reads 2^depth - 1.

The kernels' tile is 32 rows x (256 / step, 64 at step 3) samples with a halo of 3 samples and 3 field rows: the shapes below are the
planes with no edge, the plane whose only edge is at its last sample, one tile plus a row and a column, and two tiles each way with a
ragged rest.
"""
import numpy as np

BLOCKS = (4, 8, 16)
MODES = ("weak", "strong")
DEPTHS = (8, 10, 12)
THRESHOLDS = ((0, 0), (25, 13), (255, 255))
COVER_SHAPE = (40, 72)
NO_EDGE = ((1, 1), (1, 40), (40, 1), (7, 7))          # (at block 8 a row of 40 has edges; the column of 40 x 1 has none across)
LAST_SAMPLE = (9, 9)          # the edge at 8 is the last sample: Q1 and Q2 are clamped reads, their writes are dropped
TILE_ROWS = 32


def tile_cols(step: int = 1) -> int:
    return 64 if step == 3 else 256 // step


def one_tile_plus(step: int = 1):
    return TILE_ROWS + 1, tile_cols(step) + 1


def two_tiles_ragged(step: int = 1):
    return 2 * TILE_ROWS + 5, 2 * tile_cols(step) + 7


def case_plane(rng, rows: int, cols: int, depth: int = 8, above: bool = False, block: int = 8) -> np.ndarray:
    """[rows, cols] samples (uint8 at depth 8, uint16 above) of the module docstring's picture."""
    top, s = (1 << depth) - 1, 1 << (depth - 8)
    y, x = np.mgrid[0:rows, 0:cols]
    offs = rng.integers(-20, 21, (rows // block + 1, cols // block + 1))
    m = 128 + 40 * np.sin(x / 9.0) * np.cos(y / 7.0) + offs[y // block, x // block] + rng.normal(0, 1, (rows, cols))
    m = m + (x >= 2 * cols // 3) * rng.normal(0, 10, (rows, cols))
    m = np.clip(np.rint(m * s), 0, top).astype(np.int64)
    if rows >= 3 and cols >= block + 3:
        m[1, block - 3:block + 3] = top
        m[1, block - 1] = top - 8 * s
        m[2, block - 3:block + 3] = 0
        m[2, block - 1] = 8 * s
    if above and depth > 8:
        m[::2, ::5] = 60000
    return m.astype(np.uint8 if depth == 8 else np.uint16)


def noise_plane(rng, rows: int, cols: int, depth: int = 8) -> np.ndarray:
    """Uniform noise over the whole range: with thresholds (255, 255) nearly every edge is filtered and clamps fire at both ends."""
    return rng.integers(0, 1 << depth, (rows, cols)).astype(np.uint8 if depth == 8 else np.uint16)


def case_frames(rng, n: int, rows: int, cols: int, step: int = 1, depth: int = 8, above: bool = False, block: int = 8, noise: bool = False) -> np.ndarray:
    """[n, rows, cols, step] samples: a plane of its own per frame and channel."""
    one = (lambda: noise_plane(rng, rows, cols, depth)) if noise else (lambda: case_plane(rng, rows, cols, depth, above, block))
    return np.stack([np.stack([one() for _ in range(step)], -1) for _ in range(n)])


def as_bytes(m: np.ndarray) -> np.ndarray:
    """[n, ...] samples -> [n, bytes] uint8 (little-endian words for 16-bit samples)."""
    n = m.shape[0]
    return (np.ascontiguousarray(m).astype("<u2").view(np.uint8) if m.dtype != np.uint8 else np.ascontiguousarray(m)).reshape(n, -1)


def blocky_picture():
    """The blocking test's picture: (clean float64 [48, 64], blocky uint8): the clean picture plus an offset in -4 .. 4 per 8 x 8 block."""
    y, x = np.mgrid[0:48, 0:64]
    clean = 128 + 60 * np.sin(x / 11.0) * np.cos(y / 13.0)
    offs = np.random.default_rng(0).integers(-4, 5, (6, 8))
    return clean, np.clip(np.rint(clean + offs[y // 8, x // 8]), 0, 255).astype(np.uint8)
