"""Inputs of the combed= tests, shared by tests/test_combed.py (the specification) and tests/test_gpu_combed.py (the kernels and the calls
against the specification): the films of tests/pulldown_cases.py, a moving sinusoid whose fields never fit each other, and the hybrid
constructor -- telecined film, then truly interlaced video, then telecined film -- in every frame kind.

Like the films, the sinusoid is vertically flat within a field time, so every bit of combing in a woven frame comes from weaving two
moments, which is what the comb rule measures."""
import numpy as np

from savsr_amd import pulldown as pd
from savsr_amd import yuv
from tests.pulldown_cases import matrix_film

HYBRID = (8, 6, 8)                                # film frames (10 video frames), interlaced video frames, film frames (10 video frames)
SIZES = [(9, 33), (16, 16), (33, 50), (48, 64)]   # h x w


def sinusoid(m, r, c, step=1):
    """[m, r, c] uint8: 128 + 100 sin(2 pi (x - 2 k) / 24) in pixels of `step` samples: a wave of 24 pixels moving 2 pixels per picture.
    Two neighbouring pictures differ by up to 52, far above the comb threshold, in most columns; the motion is everywhere, so both
    deinterlacers interpolate within the field and a cleaned frame is exactly one picture (it reads 0 combed samples)."""
    k, _, x = np.mgrid[0:m, 0:r, 0:c]
    return np.rint(128 + 100 * np.sin(2 * np.pi * (x // step - 2 * k) / 24)).astype(np.uint8)


def moving(kind, m, r, c, step=1):
    return sinusoid(m, r, c, step) if kind == "sinusoid" else matrix_film(kind, m, r, c, step)


def packed(kind, m, h, w, c=3):
    """[m, h, w, c] uint8 pictures: the kind on the h x (w * c) byte matrix."""
    return moving(kind, m, h, w * c, c).reshape(m, h, w, c)


def planar(kind, m, h, w, depth=8, layout="420"):
    """[m, frame_bytes] uint8 pictures: every plane is the kind at the plane's size."""
    sizes = [(h, w)] if layout == yuv.MONO else [(h, w)] + [yuv.chroma_hw(h, w, layout)] * 2
    planes = [moving(kind, m, r, c).astype(np.uint16) << (depth - 8) for r, c in sizes]
    return np.concatenate([np.ascontiguousarray(p.astype(np.uint8 if depth == 8 else "<u2")).reshape(m, -1).view(np.uint8) for p in planes], 1)


def interlace(pictures, order, pixel_format="rgb", size=None, depth=8):
    """Truly interlaced video of 2 n pictures at the field rate: frame k weaves the first field of picture 2 k and the second of 2 k + 1."""
    n = pictures.shape[0] // 2
    return pd._weave_sources(pictures, order, list(range(0, 2 * n, 2)), list(range(1, 2 * n, 2)), pixel_format, size, depth)


def hybrid(order, h, w, kind="gradient", fmt="rgb", depth=8, parts=HYBRID, phase=0):
    """(frames, the indices of the truly interlaced ones): telecined `kind` film, interlaced moving sinusoid, telecined film again.
    fmt "rgb": [N, h, w, 3] uint8; "i420" / "i422" / "i444" / "y400": planar frames of that depth."""
    a, v, b = parts
    if fmt == "rgb":
        make, kw = (lambda k, m: packed(k, m, h, w)), {}
    else:
        layout = {"i420": "420", "i422": "422", "i444": "444", "y400": yuv.MONO}[fmt]
        make, kw = (lambda k, m: planar(k, m, h, w, depth, layout)), dict(pixel_format=fmt, size=(h, w), depth=depth)
    head = pd.telecine(make(kind, a), order, phase, **kw)
    mid = interlace(make("sinusoid", 2 * v), order, **kw)
    tail = pd.telecine(make(kind, b), order, 0, **kw)
    n0 = head.shape[0]
    return np.concatenate([head, mid, tail], 0), list(range(n0, n0 + mid.shape[0]))
