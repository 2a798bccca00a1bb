"""Inputs of the scan-detection tests, shared by tests/test_scan.py (the specification and its decision rule) and tests/test_gpu_scan.py
(the kernels and the calls against the specification).

The decision is tested on smooth moving pictures: a deterministic sum of sinusoids that shifts by a fixed motion per picture.  A
progressive video is the pictures themselves; an interlaced one weaves consecutive field-rate pictures into frames (the first field
from the earlier picture); a telecined one is `pulldown.telecine` of the pictures as film.  White noise carries no temporal order
(the interlace rule may answer anything on it): it is the input of the kernel-equals-specification tests only, which are exact whatever
the data."""
import numpy as np

from savsr_amd import pulldown as pd
from savsr_amd import yuv

SIZES = [(9, 17), (12, 20), (36, 48)]             # R x C
MOTIONS = [(1, 0), (0, 1), (2, 1)]                # (dx, dy) samples per picture
NOISES = (0, 2)
N_FRAMES = 12
# The telecine rule asks for two cadence hits, and a hit is a pair of frames (n, n + 2) with 1 <= n <= N - 3 that comes once in five
# frames: N - 3 >= 10 puts two of them inside the video at every phase, so the telecined cases have 13 frames (12 show one hit only at
# phases 2 .. 4).  14 film frames are 35 fields, 17 video frames: 13 are left after the 4 that the largest phase drops.
N_TELECINE = 13
N_FILM = 14
PHASES = (0, 1, 2, 3, 4)
# (amplitude, cycles per sample along x, along y, phase): low frequencies, so that neighbouring rows of one picture fit each other
WAVES = ((50.0, 0.043, 0.031, 0.3), (34.0, -0.027, 0.058, 1.1), (22.0, 0.081, -0.017, 2.0), (14.0, 0.012, 0.094, 4.4))


def pictures(m, r, c, motion=(1, 0), noise=0, seed=0):
    """[m, r, c] uint8: picture t is the sum of sinusoids sampled at (x - dx t, y - dy t), rounded; noise: uniform integers in
    [-noise, noise] added to every sample (seeded), the result clipped to 0 .. 255."""
    dx, dy = motion
    t, y, x = np.mgrid[0:m, 0:r, 0:c].astype(np.float64)
    v = np.full((m, r, c), 128.0)
    for amp, fx, fy, ph in WAVES:
        v += amp * np.sin(2 * np.pi * (fx * (x - dx * t) + fy * (y - dy * t)) + ph)
    v = np.rint(v).astype(np.int64)
    if noise:
        v += np.random.RandomState(seed).randint(-noise, noise + 1, size=v.shape)
    return np.clip(v, 0, 255).astype(np.uint8)


def weave_fields(pics, order):
    """[2 n, r, c] field-rate pictures -> [n, r, c] interlaced frames: frame k has the rows of the order's first parity from picture 2 k
    and the others from picture 2 k + 1."""
    p = pd.first_parity(order)
    pics = np.asarray(pics)
    out = pics[0::2].copy()
    out[:, 1 - p::2] = pics[1::2][:, 1 - p::2]
    return out


def matrix_case(kind, order, r, c, motion=(1, 0), noise=0, phase=0, n=N_FRAMES):
    """[n, r, c] uint8 matrices of one case ([N_TELECINE, r, c] for "telecine").  kind: "progressive", "interlaced", "telecine", "static"."""
    if kind == "progressive":
        return pictures(n, r, c, motion, noise)
    if kind == "interlaced":
        return weave_fields(pictures(2 * n, r, c, motion, noise), order)
    if kind == "telecine":
        return _telecine(pictures(N_FILM, r, c, motion, noise), order, phase)[:N_TELECINE]
    if kind == "static":
        return np.repeat(pictures(1, r, c, motion, noise), n, 0)
    raise ValueError(kind)


def _telecine(film, order, phase):
    """pulldown.telecine on [m, r, c] matrices (as packed frames of one channel)."""
    return pd.telecine(film[..., None], order, phase)[..., 0]


def expected(kind, order):
    """The verdicts (scan, order) a case may give."""
    if kind == "progressive":
        return (("progressive", None), ("undetermined", None))
    if kind == "static":
        return (("undetermined", None),)
    return ((kind, order),)


def packed_case(kind, order, h, w, c=3, **kw):
    """[n, h, w, c] uint8 frames: the case on the h x (w * c) byte matrix."""
    m = matrix_case(kind, order, h, w * c, **kw)
    return m.reshape(m.shape[0], h, w, c)


def planar_case(kind, order, h, w, depth=8, layout="420", **kw):
    """[n, frame_bytes] uint8 frames: every plane is the case at the plane's size."""
    shift = depth - 8
    sizes = [(h, w)] if layout == yuv.MONO else [(h, w)] + [yuv.chroma_hw(h, w, layout)] * 2
    planes = [matrix_case(kind, order, r, c, **kw).astype(np.uint16) << shift for r, c in sizes]
    n = planes[0].shape[0]
    return np.concatenate([np.ascontiguousarray(p.astype(np.uint8 if depth == 8 else "<u2")).reshape(n, -1).view(np.uint8) for p in planes], 1)


def noise_mats(n, r, c, top=255, seed=0):
    return np.random.RandomState(seed).randint(0, top + 1, size=(n, r, c))
