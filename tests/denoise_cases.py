"""Shared by tests/test_denoise.py, tests/test_gpu_denoise.py and tools/check_denoise_host.py: the generator of videos on which the temporal
denoiser's rule (savsr_amd/denoise.py) takes every path, and the shapes the kernels are run at.

`walk_video`: a random walk per sample.  With A = a << (depth - 8): each step is drawn from -(A / 2 + 1) .. A / 2 + 1 and taken with
probability 0.6; with probability 0.08 a jump of up to +-(4 A + 4) is added; the result is clipped to the range.  The first `static`
columns are static, the next `static` ones static with one jump to top - value at a random frame.  With N = 2 r + 6 frames of 5 x 33,
strength (4, 9) and 8 static columns it produces every tap count k = 1 .. 2 r + 1 at depth 8, 10 and 12 for r in {1, 2, 4, 16}, and
both stop reasons for r >= 4; at r <= 2 the B stop cannot fire with (4, 9) (two differences <= 4 sum to at most 8), so those radii also
run with strength (4, 5).
"""
import numpy as np

RADII = (1, 2, 4, 16)
DEPTHS = (8, 10, 12)
STRENGTH = (4, 9)
TIGHT = (4, 5)               # the strength at which the B stop fires at r <= 2
COVER_SHAPE = (5, 33)        # R x C of the coverage videos
# R x C of the kernels' runs: one sample, a ragged plane, the coverage shape, and planes of 128 / 816 / 432 bytes at 8 bits (the vector
# form where the base is aligned: one partial workgroup, more than one workgroup at 16 bits, a partial last wave)
MATRICES = ((1, 1), (2, 7), (5, 33), (4, 32), (3, 272), (9, 48))


def frames_for(r: int) -> int:
    return 2 * r + 6


def lengths_for(r: int):
    """The video lengths the entries run at: shorter than the radius, at it, past it, and the coverage length."""
    return sorted({1, 2, 3, r, r + 1, frames_for(r)})


def walk_video(rng, n: int, rows: int, cols: int, depth: int = 8, a: int = STRENGTH[0], static=None) -> np.ndarray:
    """[n, rows, cols] samples (uint8 at depth 8, uint16 above) of the module docstring's random walk.  static: the number of static
    columns and of static-with-one-jump columns (default: min(8, cols // 4))."""
    top = (1 << depth) - 1
    A = a << (depth - 8)
    s, j = A // 2 + 1, 4 * A + 4
    st = min(8, cols // 4) if static is None else static
    m = np.empty((n, rows, cols), dtype=np.int64)
    m[0] = rng.integers(0, top + 1, (rows, cols))
    for t in range(1, n):
        step = rng.integers(-s, s + 1, (rows, cols)) * (rng.random((rows, cols)) < 0.6)
        jump = rng.integers(-j, j + 1, (rows, cols)) * (rng.random((rows, cols)) < 0.08)
        m[t] = np.clip(m[t - 1] + step + jump, 0, top)
    m[:, :, :st] = m[0, :, :st]
    if n > 1 and st:
        v = m[0, :, st:2 * st]
        at = rng.integers(1, n, v.shape)
        for t in range(n):
            m[t, :, st:2 * st] = np.where(t >= at, top - v, v)
    return m.astype(np.uint8 if depth == 8 else np.uint16)


def cover_video(r: int, depth: int, seed: int = 0) -> np.ndarray:
    """The coverage video of radius r at `depth`: 2 r + 6 frames of 5 x 33."""
    return walk_video(np.random.default_rng(1000 * seed + 100 * r + depth), frames_for(r), *COVER_SHAPE, depth)


def as_bytes(m: np.ndarray) -> np.ndarray:
    """[n, R, C] samples -> [n, bytes] uint8 (little-endian words for 16-bit samples)."""
    n = m.shape[0]
    return (m.astype("<u2").view(np.uint8) if m.dtype != np.uint8 else m).reshape(n, -1)
