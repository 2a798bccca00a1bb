"""Inputs of the bwdif deinterlacer's tests, shared by tests/test_bwdif.py (the specification against a scalar loop, the branch-count
guard) and tests/test_gpu_bwdif.py (the kernels against the specification on the same inputs)."""
import numpy as np

from tests.deinterlace_cases import input_set  # noqa: F401  (the inputs are the yadif tests': static, noise, diagonals, bar)

# R x C of the matrices, the smallest at which the rule changes: no `inner` row (2, 3 rows); `inner` but no `line` row (5 rows; 8 rows
# of 16 bytes: the vector form); exactly one `line` row, y = 4, in the field that interpolates the even rows (9 rows of 33: the
# one-sample form); y = 5 for the other field (10 rows of 32: the vector form); a mid-sized vector shape; more than one column tile
# (256 bytes) and more than one row tile (32 rows)
SHAPES = [(2, 1), (3, 1), (5, 7), (8, 16), (9, 33), (10, 32), (13, 48), (33, 272)]
ORDERS = ("tff", "bff")


def inputs(r, c, top=255):
    """[(name, [3, r, c] int64 samples in 0 .. top)] of one shape."""
    return input_set(r, c, 1, top)


def zone_plate(order, h=64, w=96, fields=16):
    """A moving zone plate: (the [fields, h, w] uint8 progressive truth at the field times t, the [fields / 2, h, w] interlaced frames woven
    from it: frame n has the rows of the order's first parity from time 2 n and the others from time 2 n + 1)."""
    t, y, x = np.mgrid[0:fields, 0:h, 0:w].astype(np.float64)
    v = np.rint(128 + 100 * np.sin(0.5 * np.pi * ((x - 48 - 1.5 * t) ** 2 + (y - 32 - 0.7 * t) ** 2) / 96))
    truth = np.clip(v, 0, 255).astype(np.uint8)
    p = 0 if order == "tff" else 1
    woven = truth[0::2].copy()
    woven[:, 1 - p::2] = truth[1::2][:, 1 - p::2]
    return truth, woven


def psnr(a, b, top=255):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return float("inf") if mse == 0 else float(10 * np.log10(top * top / mse))
