"""Shared by tests/test_nlmeans.py, tests/test_gpu_nlmeans.py and tools/check_nlmeans_host.py: the generator of planes on which the spatial
denoiser's rule (savsr_amd/nlmeans.py) takes every path, and the shapes the kernels are run at.

`case_plane`: a smooth pattern with a step edge (128 + 50 sin(x / 3) cos(y / 4) + 60 [x > C / 2]) plus sigma = 2 noise, in 8-bit units
scaled to the depth, with a constant block in the top-left third (equal patches away from the centre: k = 0 off-centre) -- on 24 x 40 at
the defaults it fills k = 0 off-centre, the middle buckets and k >= 577 (tests/test_nlmeans.py checks the counts).  `above=True` also
sets every (2 y, 5 x) sample of a 16-bit plane above 2^depth - 1, where the rule reads 2^depth - 1.

The kernels' tile is 64 rows (four strips of 16) x (64 - 2 P) columns with a halo of S + P: the shapes below are the planes smaller than
the halo, one tile plus a row and a column, and two tiles each way with a ragged rest.
"""
import numpy as np

PATCHES = (1, 2, 3)
SEARCHES = (1, 3, 7)
DEPTHS = (8, 10, 12)
COVER_SHAPE = (24, 40)
TINY = ((1, 1), (1, 40), (40, 1), (3, 5))
TILE_ROWS = 64
MAX_DIVISOR = 50176          # 49 * 32^2: the largest divisor a caller can ask for


def tile_cols(patch: int) -> int:
    return 64 - 2 * patch


def one_tile_plus(patch: int):
    return TILE_ROWS + 1, tile_cols(patch) + 1


def two_tiles_ragged(patch: int):
    return 2 * TILE_ROWS + 5, 2 * tile_cols(patch) + 7


def case_plane(rng, rows: int, cols: int, depth: int = 8, above: bool = False) -> np.ndarray:
    """[rows, cols] samples (uint8 at depth 8, uint16 above) of the module docstring's picture."""
    top, s = (1 << depth) - 1, 1 << (depth - 8)
    y, x = np.mgrid[0:rows, 0:cols]
    m = (128 + 50 * np.sin(x / 3.0) * np.cos(y / 4.0) + 60 * (x > cols // 2) + rng.normal(0, 2, (rows, cols))) * s
    m = np.clip(np.rint(m), 0, top).astype(np.int64)
    m[:max(rows // 3, 1), :max(cols // 3, 1)] = 77 * s
    if above and depth > 8:
        m[::2, ::5] = 60000
    return m.astype(np.uint8 if depth == 8 else np.uint16)


def case_frames(rng, n: int, rows: int, cols: int, step: int = 1, depth: int = 8, above: bool = False) -> np.ndarray:
    """[n, rows, cols, step] samples: a plane of its own per frame and channel."""
    return np.stack([np.stack([case_plane(rng, rows, cols, depth, above) for _ in range(step)], -1) for _ in range(n)])


def as_bytes(m: np.ndarray) -> np.ndarray:
    """[n, ...] samples -> [n, bytes] uint8 (little-endian words for 16-bit samples)."""
    n = m.shape[0]
    return (np.ascontiguousarray(m).astype("<u2").view(np.uint8) if m.dtype != np.uint8 else np.ascontiguousarray(m)).reshape(n, -1)


def synthetic_picture():
    """The noise-reduction test's picture: (clean float64 [48, 64], noisy uint8)."""
    y, x = np.mgrid[0:48, 0:64]
    clean = 128 + 60 * np.sin(x / 5.0) * np.cos(y / 7.0) + 40 * (x > 32)
    noisy = np.clip(np.rint(clean + np.random.default_rng(0).normal(0, 2, clean.shape)), 0, 255).astype(np.uint8)
    return clean, noisy
