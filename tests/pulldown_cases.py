"""Inputs of the pulldown tests, shared by tests/test_pulldown.py (the specification's recovery property) and tests/test_gpu_pulldown.py
(the kernels and the calls against the specification).

Film inputs are vertically coherent, so that a frame's own field fits between its vertical neighbours and a foreign one does not: that
is what the field matcher measures.  Random noise is the wrong input for the recovery property (the fields of one noise frame are no
closer than the fields of two); it is the right one for "kernel equals specification", which is exact whatever the data."""
import numpy as np

from savsr_amd import yuv

SIZES = [(4, 5), (5, 3), (9, 33), (16, 16)]          # h x w
FILM_LENGTHS = (4, 8, 12)
KINDS = ("gradient", "bar")


def gradient(m, r, c):
    """[m, r, c] uint8: the diagonal gradient (7 y + 5 x + 11 k) mod 256."""
    k, y, x = np.mgrid[0:m, 0:r, 0:c]
    return ((7 * y + 5 * x + 11 * k) % 256).astype(np.uint8)


def bar(m, r, c, step=1):
    """[m, r, c] uint8: a bright bar two pixels (of `step` samples) wide on a flat ground, moving two pixels per film frame and wrapping."""
    v = np.full((m, r, c), 40, np.uint8)
    px = np.arange(c) // step
    w = max(c // step, 1)
    for k in range(m):
        v[k][:, (px == (2 * k) % w) | (px == (2 * k + 1) % w)] = 220
    return v


def matrix_film(kind, m, r, c, step=1):
    return gradient(m, r, c) if kind == "gradient" else bar(m, r, c, step)


def packed_film(kind, m, h, w, c=3):
    """[m, h, w, c] uint8 film frames: the kind on the h x (w * c) byte matrix."""
    return matrix_film(kind, m, h, w * c, c).reshape(m, h, w, c)


def planar_film(kind, m, h, w, depth=8, layout="420"):
    """[m, frame_bytes] uint8 film frames: every plane is the kind at the plane's size, so the chroma comes from the same film."""
    shift = depth - 8
    sizes = [(h, w)] if layout == yuv.MONO else [(h, w)] + [yuv.chroma_hw(h, w, layout)] * 2
    planes = [matrix_film(kind, m, r, c).astype(np.uint16) << shift for r, c in sizes]
    return np.concatenate([np.ascontiguousarray(p.astype(np.uint8 if depth == 8 else "<u2")).reshape(m, -1).view(np.uint8) for p in planes], 1)


def noise_mats(n, r, c, top=255, seed=0):
    return np.random.RandomState(seed).randint(0, top + 1, size=(n, r, c))
