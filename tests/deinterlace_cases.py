"""Inputs of the deinterlacer's tests, shared by tests/test_deinterlace.py (the specification against a scalar loop, the branch-count
guard) and tests/test_gpu_deinterlace.py (the kernels against the specification on the same inputs)."""
import numpy as np

# R x C of the matrices: two and three rows of one column, one row pair, no column / exactly one column / many columns that pass x +- 3
SHAPES = [(2, 1), (3, 1), (2, 7), (5, 6), (5, 7), (9, 33)]
STEPS = (1, 3)
N_FRAMES = 3


def shapes_for(step):
    """SHAPES with the columns as pixels of `step` samples, so that x +- 3 step passes for the same pixels."""
    return [(r, c * step) for r, c in SHAPES]


def static(r, c, top=255, seed=0):
    """The same random picture three times: p2 = n2, so t0 = 0."""
    return np.repeat(np.random.RandomState(seed).randint(0, top + 1, size=(1, r, c)), N_FRAMES, 0)


def noise(r, c, top=255, seed=1):
    return np.random.RandomState(seed).randint(0, top + 1, size=(N_FRAMES, r, c))


def diagonals(r, c, step=1, top=255, seed=2):
    """Frame k is g * (x + j y) over the pixels, j = -2, 1, 2 (and -1 in its lower half), plus noise in -1 .. 1: constant along the
    direction CHECK(j) compares, so CHECK(+-1) and then CHECK(+-2) win over the vertical pair."""
    rng = np.random.RandomState(seed)
    px = np.arange(c) // step
    y = np.arange(r)[:, None]
    g = max(1, top // (4 * (c // step + 2 * r)))
    out = []
    for j in (-2, 1, 2):
        jj = np.where(y >= r // 2, -1, j) if j == -2 else j
        v = g * (px[None, :] + jj * y)
        out.append(v - v.min() + 1)
    return np.clip(np.stack(out) + rng.randint(-1, 2, size=(N_FRAMES, r, c)), 0, top)


def moving_bar(r, c, step=1, top=255, order="tff"):
    """A bright bar two pixels wide on a dark ground, moving two pixels per field: the field of parity p of frame n is taken at time
    2 n + f, f = p for tff and 1 - p for bff."""
    v = np.full((N_FRAMES, r, c), top // 8)
    px = np.arange(c) // step
    for n in range(N_FRAMES):
        for p in (0, 1):
            t = 2 * n + (p if order == "tff" else 1 - p)
            v[n, p::2, (px >= 2 * t) & (px < 2 * t + 2)] = top - top // 8
    return v


def input_set(r, c, step=1, top=255):
    """[(name, [N_FRAMES, r, c] int64 samples in 0 .. top)]: what the branch-count guard and the GPU tests run."""
    return [("static", static(r, c, top)), ("noise", noise(r, c, top)), ("diagonals", diagonals(r, c, step, top)),
            ("bar", moving_bar(r, c, step, top))]
