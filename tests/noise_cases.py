"""Shared by tests/test_noise.py, tests/test_gpu_noise.py and tools/check_noise_host.py: the pictures the noise estimator
(savsr_amd/noise.py) is decided on, and the shapes its kernels (csrc/noise.hip) are run at.

`picture`: 128 + 60 sin(x / 11) cos(y / 13) plus sigma white Gaussian noise, scaled to the depth and rounded; bars: the first and the
last eighth of the rows are a constant 16 (a quarter of the frame, as a letterbox).  Every case has its own seed, fixed here.

The statistics kernel gives every 8 x 8 cell (support 10 x 10 samples) a lane and a workgroup 256 lanes; the vector form needs rows of a
multiple of 8 bytes (16 for 16-bit samples) at step 1.  `stats_tile` is a plane whose cells fill exactly one workgroup.
"""
import numpy as np

SEED = 5
LARGE_SHAPE = (288, 352)
SMALL_SHAPE = (96, 128)
SIGMAS = (1, 2, 4, 8)
CELL = 8
STATS_LANES = 256
SMALLEST = ((9, 9), (10, 10), (10, 18), (10, 26), (18, 10), (9, 40))          # the first and the last have no cell


def case_seed(*key) -> int:
    """One seed per case, from SEED and the case's numbers."""
    s = SEED
    for k in key:
        s = s * 1009 + int(k) + 1
    return s


def picture(seed: int, rows: int, cols: int, sigma: float = 0.0, depth: int = 8, bars: bool = False) -> np.ndarray:
    """[rows, cols] samples (uint8, or uint16 at depth 10 / 12) of the module docstring's picture; sigma in 8-bit code units."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols]
    m = 128 + 60 * np.sin(x / 11.0) * np.cos(y / 13.0)
    if sigma:
        m = m + rng.normal(0, sigma, (rows, cols))
    m = np.clip(np.rint(m * (1 << (depth - 8))), 0, (1 << depth) - 1)
    if bars:
        m[:rows // 8] = m[rows - rows // 8:] = 16 << (depth - 8)
    return m.astype(np.uint8 if depth == 8 else np.uint16)


def true_sigma(sigma: float) -> float:
    """What the estimator should read on `picture` at depth 8: the noise and the rounding's 1/12 together."""
    return float(np.sqrt(sigma * sigma + 1.0 / 12.0))


def checkerboard(rows: int, cols: int) -> np.ndarray:
    """uint8 0 / 255 by (x + y) parity: every L is 2040, every cell sums to 130560 and lands in row 254."""
    y, x = np.mgrid[0:rows, 0:cols]
    return (255 * ((x + y) % 2)).astype(np.uint8)


def stats_plane(rng, rows: int, cols: int, depth: int = 8, above: bool = False) -> np.ndarray:
    """[rows, cols] samples whose cells spread over many rows of the table and are flat here and there: a smooth slope plus noise whose
    amplitude grows along the rows, a constant patch on every third 16 x 16 tile, scaled to the depth; above: every (2 y, 5 x) sample of
    a 16-bit plane lies above 2^depth - 1."""
    y, x = np.mgrid[0:rows, 0:cols]
    amp = 1 + (x // 8) % 13
    m = 100 + 30 * np.sin(x / 7.0) * np.cos(y / 5.0) + rng.integers(-64, 65, (rows, cols)) * amp / 16.0
    m = np.where((x // 16 + y // 16) % 3 == 0, 90.0, m)
    m = np.clip(np.rint(m * (1 << (depth - 8))), 0, (1 << depth) - 1).astype(np.int64)
    if above and depth > 8:
        m[::2, ::5] = 60000
    return m.astype(np.uint8 if depth == 8 else np.uint16)


def stats_frames(rng, n: int, rows: int, cols: int, step: int = 1, depth: int = 8, above: bool = False) -> np.ndarray:
    """[n, rows, cols, step] samples: a plane of its own per frame and channel."""
    return np.stack([np.stack([stats_plane(rng, rows, cols, depth, above) for _ in range(step)], -1) for _ in range(n)])


def stats_tile():
    """(rows, cols) of a plane of 16 x 16 cells: one workgroup of the kernel; cols is a multiple of 16 less 2, so add 2 for the vector form."""
    return CELL * 16 + 2, CELL * 16 + 2


def flat_beside_binned() -> np.ndarray:
    """uint8 [10, 18]: the cell on the left is constant (flat), the one on the right is noise (binned)."""
    m = np.full((10, 18), 77, np.uint8)
    m[:, 9:] = np.random.default_rng(case_seed(10, 18)).integers(0, 256, (10, 9))
    return m
