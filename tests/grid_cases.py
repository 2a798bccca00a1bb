"""Shared by tests/test_grid.py, tests/test_gpu_grid.py and tools/check_grid_host.py: the pictures the grid detector
(savsr_amd/grid.py) is decided on, and the shapes its kernels (csrc/grid.hip) and the origin path of csrc/deblock.hip are run at.

`blocky`: 128 + 60 sin(x / 11) cos(y / 13) plus an offset in -a .. a per `block` x `block` block plus sigma noise, drawn with the grid at
the picture's origin on a canvas one block larger each way and then cropped by (block - o) % block rows and columns, so that the grid of
the rows x cols picture that comes back sits at origin (oy, ox).  block None: no offsets.  Every case has its own seed, fixed here.

The statistics kernel works on bands of 4 rows (of a field, in field mode) x 256 lanes; a lane of the 16-byte form owns 16 bytes of a
row, a lane of the one-sample form one sample.  `stats_tile` is that tile for a plane of bytes at step 1 in the 16-byte form.
"""
import numpy as np

SEED = 3
DECISION_SHAPE = (288, 352)
BLOCKY = ((8, 4, 0), (8, 4, 1), (8, 6, 2), (16, 4, 0), (16, 4, 1), (16, 6, 2), (4, 4, 1), (4, 6, 2))          # (block, a, sigma)
CLEAN_SIGMAS = (0, 1, 2, 4)
STATS_BAND = 4
STATS_LANES = 256


def origins(block: int):
    return ((0, 0), (3, 5) if block > 4 else (3, 1), (block - 1, 1))


def case_seed(*key) -> int:
    """One seed per case, from SEED and the case's numbers."""
    s = SEED
    for k in key:
        s = s * 1009 + int(k) + 1
    return s


def blocky(seed: int, rows: int, cols: int, block=None, a: int = 4, sigma: float = 0.0, origin=(0, 0), interlaced: bool = False) -> np.ndarray:
    """uint8 [rows, cols] of the module docstring's picture.  interlaced: the picture is frame-coded all the same (the blocks span both
    fields); the argument is there so that a case reads as what it is."""
    rng = np.random.default_rng(seed)
    b = block or 16
    R, C = rows + b, cols + b
    y, x = np.mgrid[0:R, 0:C]
    m = 128 + 60 * np.sin(x / 11.0) * np.cos(y / 13.0)
    if block:
        offs = rng.integers(-a, a + 1, (R // b + 1, C // b + 1))
        m = m + offs[y // b, x // b]
    if sigma:
        m = m + rng.normal(0, sigma, (R, C))
    m = np.clip(np.rint(m), 0, 255).astype(np.uint8)
    cy, cx = ((b - origin[0]) % b, (b - origin[1]) % b) if block else (0, 0)
    return np.ascontiguousarray(m[cy:cy + rows, cx:cx + cols])


def uniform_noise(seed: int, rows: int, cols: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (rows, cols)).astype(np.uint8)


def stats_plane(rng, rows: int, cols: int, depth: int = 8, above: bool = False) -> np.ndarray:
    """[rows, cols] samples on which about one boundary in five is a hit each way: a smooth slope plus steps of a few codes and noise,
    scaled to the depth; above: every (2 y, 5 x) sample of a 16-bit plane lies above 2^depth - 1."""
    y, x = np.mgrid[0:rows, 0:cols]
    m = 100 + 30 * np.sin(x / 7.0) * np.cos(y / 5.0) + rng.integers(-6, 7, (rows, cols)) + 5 * ((x // 8 + y // 8) % 2)
    m = np.clip(np.rint(m * (1 << (depth - 8))) + (rng.integers(0, 1 << (depth - 8), (rows, cols)) if depth > 8 else 0), 0, (1 << depth) - 1).astype(np.int64)
    if above and depth > 8:
        m[::2, ::5] = 60000
    return m.astype(np.uint8 if depth == 8 else np.uint16)


def stats_frames(rng, n: int, rows: int, cols: int, step: int = 1, depth: int = 8, above: bool = False) -> np.ndarray:
    """[n, rows, cols, step] samples: a plane of its own per frame and channel."""
    return np.stack([np.stack([stats_plane(rng, rows, cols, depth, above) for _ in range(step)], -1) for _ in range(n)])


def stats_tile(step: int = 1, sample: int = 1):
    """(rows, cols in pixels) of one workgroup of the 16-byte form: 4 rows x (256 lanes x 16 bytes) of a row when the row is that long."""
    return STATS_BAND, STATS_LANES * 16 // (sample * step)
