"""Temporal noise reduction in front of the network: the host-side specification (numpy, integers only, no GPU needed).

An SD source carries more than its picture: tape, tuner and sensor noise, and the temporal flicker MPEG-2 quantisation leaves.  A network
trained on clean downsamples reconstructs what it is shown, so noise that changes from frame to frame is enlarged with the picture.  The
stage here averages a sample with the same sample of the frames around it, as long as they stay close to it: ffmpeg `atadenoise`'s serial
algorithm (adaptive temporal averaging) with this project's border condition.  `denoise_matrix` is the rule, sample by sample, in
integers; csrc/denoise.hip equals it bit for bit.  `upscale_video(v, denoise="ata", ...)` is, bit for bit,
`upscale_video(denoise_video(v', ...), ...)`, v' the deinterlaced or pulldown-removed video: the stage runs after surface= unpacking,
scan="detect" and fields= / pulldown= (it needs progressive frames) and in front of the crop, the cuts and the windows.  The rule is per
sample, so it commutes with crop= exactly: denoising the cropped video gives the crop of the denoised one.

The rule, for one matrix m[N, R, C] of integer samples (a plane, or the h x (w * c) bytes of packed uint8 frames), radius r, thresholds
A = a << (depth - 8) and B = b << (depth - 8) (a, b in 8-bit code units), frame t and sample x = m[t]:
  walk backwards d = 1 .. r, stopping where frame t - d does not exist.  At each step diff = |x - m[t - d]| and acc += diff; stop if
    diff > A or acc > B, otherwise the tap is taken;
  walk forwards in the same way and independently, with an accumulator of its own: a dead backward walk does not end the forward one;
  out = (x + the taken taps + (k >> 1)) // k, k = 1 + the number of taken taps.
Samples at depth d are read as min(s, 2^d - 1), x included.  The two walks are independent on purpose: the first frame after a cut or a
jump still averages forwards, where atadenoise's parallel form would pass it through and let the noise pop back for r frames after
every cut.  What follows from the rule: a static sample, and exact repeats of any length, come back unchanged for every r; a sample whose
neighbours all differ by more than A comes back unchanged; |out - x| <= min(A, B) (every taken tap lies within A of x, and the taps of
one side together within B: with both sides taken k >= 3, so the mean moves by at most 2 B / 3); a = b = 0 averages exact repeats only
and is the identity.  Sums stay below 2^18 at depth 12 (33 * 4095).

How far ffmpeg is followed: the serial walk and its two thresholds are atadenoise's.  The border (a walk ends at the video's end
instead of mirroring), the rounded division and the thresholds' scale (8-bit code units, shifted to the depth) are this project's.
ffmpeg is not available where this was written, so nothing here is pinned to its output.  The defaults -- radius 4 (nine frames,
atadenoise's s=9) and strength (4, 9), roughly its 0.02 / 0.04 at 8 bits -- are parameters; nothing is validated on footage.  Temporal
only: no spatial or motion-compensated filtering, so moving texture is not denoised at all; the taps read across scene cuts, as the
deinterlacers' do, and only the thresholds stop them; one strength per video.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from .frames import check_pixel_format, layout_of
from .yuv import MONO, check_depth, frame_bytes, layout_name, luma_plane, split_planes

DENOISERS = ("ata",)
DEFAULT_RADIUS = 4
DEFAULT_STRENGTH = (4, 9)
MAX_RADIUS = 16
MAX_STRENGTH = 255
AUTO = "auto"                     # denoise_strength="auto": from the frames' noise level (savsr_amd/noise.py)


def check_denoiser(denoise, what: str = "denoise") -> Optional[str]:
    """denoise is None or one of DENOISERS."""
    if denoise is None:
        return None
    if not isinstance(denoise, str) or denoise not in DENOISERS:
        raise ValueError(f"{what} = {denoise!r}: None or one of {', '.join(DENOISERS)}")
    return denoise


def check_radius(radius, what: str = "radius") -> int:
    """1 <= radius <= 16 frames on either side."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"{what} = {radius!r}: an int in 1 .. {MAX_RADIUS} (the frames averaged on either side)")
    return int(radius)


def check_strength(strength, what: str = "strength") -> Tuple[int, int]:
    """(a, b) in 8-bit code units, 0 <= a <= b <= 255."""
    ok = isinstance(strength, (tuple, list)) and len(strength) == 2 and all(
        isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in strength)
    if not ok or not 0 <= strength[0] <= strength[1] <= MAX_STRENGTH:
        raise ValueError(f"{what} = {strength!r}: (a, b) ints in 8-bit code units with 0 <= a <= b <= {MAX_STRENGTH} (a: the largest "
                         f"difference of a tap, b: the largest sum of differences of a side)")
    return int(strength[0]), int(strength[1])


def _at_default(value, default) -> bool:
    if default is None:
        return value is None
    return isinstance(value, (tuple, list)) and tuple(value) == default if isinstance(default, tuple) else (
        not isinstance(value, bool) and isinstance(value, (int, np.integer)) and value == default)


def check_denoise_options(denoise, radius, strength, chroma_strength, prefix: str = "denoise_"):
    """The denoise= arguments of upscale_video / VideoUpscaler: None without denoise= (the options must then be at their defaults), else
    (radius, strength, chroma strength) checked; chroma_strength None: the strength.  strength "auto" (upscale_video alone: the noise
    level is measured on the frames, savsr_amd/noise.py) comes back as it is, beside the chroma strength as given."""
    if check_denoiser(denoise) is None:
        for name, value, default in ((f"{prefix}radius", radius, DEFAULT_RADIUS), (f"{prefix}strength", strength, DEFAULT_STRENGTH),
                                     (f"{prefix}chroma_strength", chroma_strength, None)):
            if not _at_default(value, default):
                raise ValueError(f"{name} = {value!r} goes with denoise=: without the stage there is nothing to set")
        return None
    r = check_radius(radius, f"{prefix}radius")
    if isinstance(strength, str) and strength == AUTO:          # found from the frames by the caller; an explicit chroma strength wins
        return r, AUTO, None if chroma_strength is None else check_strength(chroma_strength, f"{prefix}chroma_strength")
    s = check_strength(strength, f"{prefix}strength")
    return r, s, s if chroma_strength is None else check_strength(chroma_strength, f"{prefix}chroma_strength")


def denoise_matrix(mats, radius: int = DEFAULT_RADIUS, a: int = DEFAULT_STRENGTH[0], b: int = DEFAULT_STRENGTH[1], depth: int = 8,
                   return_counts: bool = False):
    """[N, R, C] integer samples -> [N, R, C] of the same dtype: the rule of the module's docstring on every sample.  return_counts:
    (the result, counts) with counts = {"k": the number of samples per tap count, an int64 array of 2 * radius + 2 entries (index k),
    "stop_a" / "stop_b" / "stop_end": the walks ended by diff > A, by acc > B (diff <= A), by the video's end}; a walk that takes all its
    `radius` taps is counted by none of them."""
    r = check_radius(radius)
    a, b = check_strength((a, b), "(a, b)")
    m = np.asarray(mats)
    if m.ndim != 3 or m.dtype.kind not in "iu":
        raise ValueError(f"matrices must be [N, R, C] integers, got {m.dtype} {tuple(m.shape)}")
    N, R, C = m.shape
    if N < 1:
        raise ValueError("the video has no frames")
    if R < 1 or C < 1:
        raise ValueError(f"a matrix of {R} x {C}: R >= 1 and C >= 1")
    if depth not in (8, 10, 12):
        raise ValueError(f"depth = {depth!r}: 8, 10 or 12")
    A, B = a << (depth - 8), b << (depth - 8)
    v = np.minimum(m.astype(np.int64), (1 << depth) - 1)
    out = np.empty_like(m)
    counts = {"k": np.zeros(2 * r + 2, dtype=np.int64), "stop_a": 0, "stop_b": 0, "stop_end": 0}
    for t in range(N):
        x = v[t]
        total, k = x.copy(), np.ones((R, C), dtype=np.int64)
        for side in (-1, 1):
            alive = np.ones((R, C), dtype=bool)
            acc = np.zeros((R, C), dtype=np.int64)
            for d in range(1, r + 1):
                u = t + side * d
                if u < 0 or u >= N:
                    counts["stop_end"] += int(np.count_nonzero(alive))
                    break
                diff = np.abs(x - v[u])
                acc = acc + diff
                stop_a = alive & (diff > A)
                stop_b = alive & ~stop_a & (acc > B)
                counts["stop_a"] += int(np.count_nonzero(stop_a))
                counts["stop_b"] += int(np.count_nonzero(stop_b))
                alive = alive & ~stop_a & ~stop_b
                total += np.where(alive, v[u], 0)
                k += alive
        out[t] = ((total + (k >> 1)) // k).astype(m.dtype)
        counts["k"] += np.bincount(k.reshape(-1), minlength=2 * r + 2)
    return (out, counts) if return_counts else out


def _planes(frames: np.ndarray, h: int, w: int, depth: int, layout: str):
    if layout == MONO:
        return [luma_plane(frames, h, w, depth, MONO)]
    return list(split_planes(frames, h, w, depth, layout))


def denoise_frames(frames, pixel_format: str = "rgb", size=None, depth: int = 8, radius: int = DEFAULT_RADIUS, strength=DEFAULT_STRENGTH,
                   chroma_strength=None) -> np.ndarray:
    """N frames -> N denoised frames in the same format: `denoise_matrix` on every matrix.  [N, h, w, c] uint8: the h x (w * c) byte matrix
    with `strength`.  Planar frames (pixel_format "i420", "i422", "i444", "y400" with size=(h, w); [N, frame_bytes] uint8, little-endian
    16-bit words at depth 10 / 12): the Y plane with `strength`, the chroma planes with `chroma_strength` (None: `strength`).  strength =
    (a, b) in 8-bit code units at every depth.  Float frames are refused."""
    r = check_radius(radius)
    s = check_strength(strength)
    cs = s if chroma_strength is None else check_strength(chroma_strength, "chroma_strength")
    hw = check_pixel_format(pixel_format, size)
    if hasattr(frames, "detach"):
        frames = frames.detach().cpu().numpy()
    frames = np.asarray(frames)
    if hw:
        h, w = hw
        layout, depth = layout_of(pixel_format), check_depth(depth)
        fb = frame_bytes(h, w, depth, layout)
        if frames.dtype != np.uint8 or frames.ndim != 2 or frames.shape[1] != fb:
            raise ValueError(f"{'' if depth == 8 else f'{depth}-bit '}{layout_name(layout)} frames of {h} x {w} are [N, {fb}] uint8, "
                             f"got {frames.dtype} {tuple(frames.shape)}")
        planes = [denoise_matrix(p, r, *(s if i == 0 else cs), depth) for i, p in enumerate(_planes(frames, h, w, depth, layout))]
        n = planes[0].shape[0]
        return np.concatenate([np.ascontiguousarray(p.astype(np.uint8 if depth == 8 else "<u2")).reshape(n, -1).view(np.uint8) for p in planes], 1)
    if depth != 8:
        raise ValueError(f"depth = {depth} goes with pixel_format = 'i420', 'i422', 'i444' or 'y400': packed frames are 8-bit")
    if frames.dtype.kind == "f":
        raise ValueError("float frames have no integer samples to denoise: give [N, h, w, c] uint8 or planar frames (quantise first)")
    if frames.dtype != np.uint8 or frames.ndim != 4:
        raise ValueError(f"frames must be [N, h, w, c] uint8, got {frames.dtype} {tuple(frames.shape)}")
    n, h, w, c = frames.shape
    return denoise_matrix(frames.reshape(n, h, w * c), r, *s, 8).reshape(n, h, w, c)


# ---- the streaming stage's indexing (prepass.TemporalDenoiser runs it on device tensors) ----------------------------------------------------
def stream_ranges(chunks, radius: int):
    """What a look-ahead window of `radius` frames on either side does with pushes of `chunks` frames each, then the end of the video:
    per step (first, count, lo, hi, held): the step's buffer holds video frames [first, first + count), its frames [lo, hi) (buffer
    indices) are final now, and `held` frames stay on the device afterwards.  The model of prepass._LookAhead(radius, radius); the tests
    check its bound (held <= 2 * radius) and that the ranges tile the video with `radius` frames of context wherever the video has them."""
    r = check_radius(radius)
    first = count = todo = 0
    steps = []
    for k in list(chunks) + [None]:
        last = k is None
        k = 0 if last else int(k)
        n = count + k
        lo = n - todo - k
        hi = n if last else max(n - r, lo)
        if last:
            keep_from, todo_next = n, 0
        elif hi > lo:
            keep_from, todo_next = max(hi - r, 0), n - hi
        else:
            keep_from, todo_next = 0, todo + k
        steps.append((first, n, lo, hi, n - keep_from))
        first, count, todo = first + keep_from, n - keep_from, todo_next
    return steps
