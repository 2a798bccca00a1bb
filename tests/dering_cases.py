"""Shared by tests/test_dering.py, tests/test_gpu_dering.py and tools/check_dering_host.py: the generators of planes on which the
deringing rule (savsr_amd/dering.py) takes every branch, and the shapes the kernels are run at.

`case_plane`: oblique edges of several slopes (so that several of the eight directions win), a disc, smooth shading and sigma = 1.5
noise, in 8-bit units scaled to the depth; the right quarter is flat apart from weak noise, so that blocks with 0 < var < 64 occur beside
blocks with var >= 64, and the bottom rows are exactly constant where the plane has room (var == 0: P8 = 0).  `above=True` also sets every
(2 y, 5 x) sample of a 16-bit plane above 2^depth - 1, where the rule reads 2^depth - 1.  `noise_plane`: uniform noise over the whole
range.  `constant_blocks`: every 8 x 8 block a constant in 100 .. 139 -- eight equal costs in every block, so the tie rule alone decides
the direction the secondary taps take across the block borders.

The kernels' tile is 32 rows x (256 / step, 64 at step 3) pixels with a halo of 2 samples and 2 field rows: the shapes below are the
smallest planes, one tile plus a row and a column, and two tiles each way with a ragged rest.
"""
import numpy as np

DEPTHS = (8, 10, 12)
STRENGTHS = ((0, 0), (0, 2), (4, 0), (15, 4), (4, 2))
DAMPINGS = (3, 6)
SMALL = ((1, 1), (1, 9), (9, 1), (7, 7), (8, 8), (9, 9))
FIELD_ROWS = (1, 2, 17)          # field-wise: fields of (1, 0), (1, 1) and (9, 8) rows
TIE_SHAPE = (40, 72)
TILE_ROWS = 32


def tile_cols(step: int = 1) -> int:
    return 64 if step == 3 else 256 // step


def one_tile_plus(step: int = 1):
    return TILE_ROWS + 1, tile_cols(step) + 1


def two_tiles_ragged(step: int = 1):
    return 2 * TILE_ROWS + 5, 2 * tile_cols(step) + 7


def case_plane(rng, rows: int, cols: int, depth: int = 8, above: bool = False) -> np.ndarray:
    """[rows, cols] samples (uint8 at depth 8, uint16 above) of the module docstring's picture."""
    top, s = (1 << depth) - 1, 1 << (depth - 8)
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    m = 100 + 0.4 * x + 0.3 * y
    m += 70 * ((x + 2 * y) % 37 < 12) - 50 * ((3 * x - y) % 53 < 9) + 40 * ((x - y) % 29 < 6) + 30 * (y % 23 < 4) - 35 * (x % 31 < 5)
    m += 60 * ((x - cols / 3.0) ** 2 + (y - rows / 2.0) ** 2 < (min(rows, cols) / 4.0) ** 2)
    m += rng.normal(0, 1.5, (rows, cols))
    flat = x >= 3 * cols // 4
    m = np.where(flat, 90 + rng.normal(0, 0.6, (rows, cols)), m)
    m = np.clip(np.rint(m * s), 0, top).astype(np.int64)
    if rows >= 24:
        m[rows - rows % 8 - 8:] = 77 * s
    if above and depth > 8:
        m[::2, ::5] = 60000
    return m.astype(np.uint8 if depth == 8 else np.uint16)


def noise_plane(rng, rows: int, cols: int, depth: int = 8) -> np.ndarray:
    """Uniform noise over the whole range."""
    return rng.integers(0, 1 << depth, (rows, cols)).astype(np.uint8 if depth == 8 else np.uint16)


def constant_blocks(rows: int = TIE_SHAPE[0], cols: int = TIE_SHAPE[1], depth: int = 8, seed: int = 0) -> np.ndarray:
    """Every 8 x 8 block a constant in 100 .. 139 (8-bit units scaled to the depth)."""
    vals = np.random.default_rng(seed).integers(100, 140, (-(-rows // 8), -(-cols // 8))) << (depth - 8)
    return np.repeat(np.repeat(vals, 8, 0), 8, 1)[:rows, :cols].astype(np.uint8 if depth == 8 else np.uint16)


def case_frames(rng, n: int, rows: int, cols: int, step: int = 1, depth: int = 8, above: bool = False, kind: str = "case") -> np.ndarray:
    """[n, rows, cols, step] samples: a plane of its own per frame and channel.  kind: "case", "noise" or "blocks"."""
    def one():
        if kind == "noise":
            return noise_plane(rng, rows, cols, depth)
        if kind == "blocks":
            return constant_blocks(rows, cols, depth, int(rng.integers(1 << 30)))
        return case_plane(rng, rows, cols, depth, above)
    return np.stack([np.stack([one() for _ in range(step)], -1) for _ in range(n)])


def as_bytes(m: np.ndarray) -> np.ndarray:
    """[n, ...] samples -> [n, bytes] uint8 (little-endian words for 16-bit samples)."""
    n = m.shape[0]
    return (np.ascontiguousarray(m).astype("<u2").view(np.uint8) if m.dtype != np.uint8 else np.ascontiguousarray(m)).reshape(n, -1)


def _dct_matrix() -> np.ndarray:
    k, n = np.mgrid[0:8, 0:8].astype(np.float64)
    d = np.cos((2 * n + 1) * k * np.pi / 16) * 0.5
    d[0] /= np.sqrt(2.0)
    return d


def ringing_picture(rows: int = 96, cols: int = 128, q: float = 40.0):
    """The ringing test's picture: (clean float64 [rows, cols], coded uint8): oblique edges, a disc and smooth shading, coded by an
    orthonormal 8 x 8 DCT whose AC coefficients are quantised with the step q (the DC with q / 4)."""
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    clean = 90 + 0.3 * x + 0.2 * y + 80 * ((x + 1.7 * y) % 61 < 24) - 50 * ((2.3 * x - y) % 83 < 30)
    clean += 60 * ((x - 80) ** 2 + (y - 50) ** 2 < 24 ** 2)
    clean = np.clip(clean, 0, 255)
    d = _dct_matrix()
    blocks = clean.reshape(rows // 8, 8, cols // 8, 8).transpose(0, 2, 1, 3) - 128
    coef = d @ blocks @ d.T
    step = np.full((8, 8), q)
    step[0, 0] = q / 4
    coded = d.T @ (np.rint(coef / step) * step) @ d + 128
    coded = coded.transpose(0, 2, 1, 3).reshape(rows, cols)
    return clean, np.clip(np.rint(coded), 0, 255).astype(np.uint8)
