"""The self-ensemble restated on the host (numpy / torch), shared by tests/test_ensemble.py and tests/test_gpu_ensemble.py.

Variant k = 0 .. 7: fw = k & 1 flips the width, fh = (k >> 1) & 1 the height, t = k >> 2 transposes the last two dims.  Forward: the
flips, then the transpose; inverse: the transpose, then the flips; merge: ((((o0 + o1) + o2) + ...) + o7) * 0.125 in fp32."""
import numpy as np


def bits(k: int):
    return k & 1, (k >> 1) & 1, k >> 2


def variant_scale(k: int, scale):
    """The scale the network runs variant k at: swapped for a transposed variant."""
    sh, sw = float(scale[0]), float(scale[1])
    return (sw, sh) if k >> 2 else (sh, sw)


def fwd_np(x: np.ndarray, k: int) -> np.ndarray:
    fw, fh, t = bits(k)
    if fw:
        x = x[..., ::-1]
    if fh:
        x = x[..., ::-1, :]
    if t:
        x = np.swapaxes(x, -1, -2)
    return np.ascontiguousarray(x)


def inv_np(y: np.ndarray, k: int) -> np.ndarray:
    fw, fh, t = bits(k)
    if t:
        y = np.swapaxes(y, -1, -2)
    if fh:
        y = y[..., ::-1, :]
    if fw:
        y = y[..., ::-1]
    return np.ascontiguousarray(y)


def fwd_t(x, k: int):
    """fwd_np for torch tensors (any device)."""
    fw, fh, t = bits(k)
    if fw:
        x = x.flip(-1)
    if fh:
        x = x.flip(-2)
    if t:
        x = x.transpose(-1, -2)
    return x.contiguous()


def inv_t(y, k: int):
    fw, fh, t = bits(k)
    if t:
        y = y.transpose(-1, -2)
    if fh:
        y = y.flip(-2)
    if fw:
        y = y.flip(-1)
    return y.contiguous()


def merge_t(outs):
    """outs[k] = variant k's network output; the inverse-transformed outputs summed in order, times 0.125."""
    acc = inv_t(outs[0], 0)
    for k in range(1, 8):
        acc = acc + inv_t(outs[k], k)
    return acc * 0.125
