"""Spatial noise reduction in front of the network: the host-side specification (numpy, integers only, no GPU needed).

`denoise="ata"` is temporal only, so grain, tuner noise and sensor noise on anything that moves reach the network untouched and are
enlarged as detail.  The stage here is non-local means (the filter of ffmpeg `nlmeans`) in this project's integer form: a sample becomes
the weighted mean of the samples around it, each weighted by how alike the patches around the two are.  `nlm_matrix` is the rule, in
integers; csrc/nlmeans.hip equals it bit for bit.  The stage is spatial only: every frame is filtered on its own.

The rule, for one matrix m[R, C] of integer samples, depth d in {8, 10, 12}, patch radius P in {1, 2, 3}, search radius S in 1 .. 7 and
an integer divisor D >= 1:
  v = min(m, 2^d - 1); coordinates outside the plane clamp to it (v[cl(y), cl(x)], the replicate-padded plane);
  for output sample p and every offset delta = (dy, dx), |dy|, |dx| <= S, whose candidate q = p + delta lies inside the plane:
    SSD = sum over |i|, |j| <= P of (v[cl(p + (i, j))] - v[cl(q + (i, j))])^2
    k = ((SSD >> 2 (d - 8)) * 64) // D
    w = WEIGHTS[k] if k < 577 else 0
  candidates outside the plane are not taken;
  out = (sum of w * v[q] + (sum of w >> 1)) // sum of w.
WEIGHTS[i] = rint(4096 * exp(-i / 64)), i = 0 .. 576: WEIGHTS[0] = 4096, WEIGHTS[576] = 1, and entry 577 would round to 0.  The value
before rounding that lies closest to a half is 1.08e-3 away from it (i = 22), so no libm can flip an entry.  The centre (delta = 0,
SSD = 0, w = 4096) is always taken, so the sum of the weights is at least 4096.  32-bit arithmetic is enough: SSD <= 49 * 4095^2 < 2^30,
(SSD >> 2 (d - 8)) * 64 < 2^28, and the numerator is at most 225 * 4096 * 4095 = 3 773 952 000, below 2^32 with the rounding term --
which is why S stops at 7.

`strength` is h, an int or float with 0 < h <= 32, in 8-bit code units at every depth: D = int(rint((2 P + 1)^2 * h^2)), refused below
1, so patches whose mean squared difference is h^2 get the weight e^-1.

What follows from the rule (tests/test_nlmeans.py holds it): a constant plane comes back unchanged; every output lies within the min /
max of the taken candidates; D = 1 on a plane without two equal patches is the identity; the rule is exactly equivariant under up/down
flip, left/right flip and transpose (clamping, the candidate set and the rounding are symmetric); it is translation-invariant at
distance >= S + P from the border.  It does not commute with a crop (a patch at the crop's edge sees clamped samples where the full frame
has picture or bars), so the stage runs after the crop.

Planar frames ("i420", "i422", "i444", "y400" at 8, 10 or 12 bits) filter every plane: Y with `strength`, chroma with `chroma_strength`
(None: the strength) and the same P and S in chroma samples.  [N, h, w, c] uint8 frames filter every channel as a plane of its own (sample
step c): a channel only meets itself.  Float frames are refused.

How far ffmpeg is followed: the patch / search structure and the exponential weight are nlmeans'.  The integer table, the border
(clamped patches, candidates outside the plane not taken), the rounding and the strength's scale are this project's; ffmpeg is not
available where this was written, so nothing here is pinned to its output.  The defaults -- P = 3, S = 7 (nlmeans' p = 7, r = 15) and
h = 3.0 -- are parameters; nothing is validated on footage (ffmpeg's default s = 1.0 is about h = 1.43 in these units, which does
nothing measurable against sigma = 2 noise on the synthetic picture of the tests).  One strength per video, no joint-channel weights,
the centre weight is not corrected for noise, and the search stops at 15 x 15.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from .frames import check_pixel_format, layout_of
from .yuv import MONO, check_depth, frame_bytes, layout_name, luma_plane, split_planes

SPATIAL_DENOISERS = ("nlm",)
DEFAULT_PATCH = 3
DEFAULT_SEARCH = 7
DEFAULT_STRENGTH = 3.0          # a parameter: nothing is validated on footage
MAX_PATCH = 3
MAX_SEARCH = 7
MAX_STRENGTH = 32
AUTO = "auto"                     # spatial_strength="auto": from the frames' noise level (savsr_amd/noise.py)
N_WEIGHTS = 577
WEIGHTS = tuple(int(np.rint(4096.0 * np.exp(-i / 64.0))) for i in range(N_WEIGHTS))


def check_spatial_denoiser(spatial_denoise, what: str = "spatial_denoise") -> Optional[str]:
    """spatial_denoise is None or one of SPATIAL_DENOISERS."""
    if spatial_denoise is None:
        return None
    if not isinstance(spatial_denoise, str) or spatial_denoise not in SPATIAL_DENOISERS:
        raise ValueError(f"{what} = {spatial_denoise!r}: None or one of {', '.join(SPATIAL_DENOISERS)}")
    return spatial_denoise


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_patch(patch, what: str = "patch") -> int:
    """1 <= patch <= 3: the patch is (2 patch + 1)^2 samples."""
    if not _is_int(patch) or not 1 <= patch <= MAX_PATCH:
        raise ValueError(f"{what} = {patch!r}: an int in 1 .. {MAX_PATCH} (the patch radius: patches of (2 P + 1)^2 samples)")
    return int(patch)


def check_search(search, what: str = "search") -> int:
    """1 <= search <= 7: the candidates lie in a (2 search + 1)^2 window."""
    if not _is_int(search) or not 1 <= search <= MAX_SEARCH:
        raise ValueError(f"{what} = {search!r}: an int in 1 .. {MAX_SEARCH} (the search radius: candidates in a (2 S + 1)^2 window)")
    return int(search)


def check_strength(strength, what: str = "strength") -> float:
    """0 < h <= 32 in 8-bit code units, an int or a float."""
    ok = (_is_int(strength) or isinstance(strength, (float, np.floating))) and np.isfinite(strength) and 0 < strength <= MAX_STRENGTH
    if not ok:
        raise ValueError(f"{what} = {strength!r}: a number with 0 < h <= {MAX_STRENGTH}, in 8-bit code units at every depth (patches whose "
                         f"mean squared difference is h^2 get the weight 1 / e)")
    return float(strength)


def divisor(patch: int = DEFAULT_PATCH, strength=DEFAULT_STRENGTH, what: str = "strength") -> int:
    """D = int(rint((2 P + 1)^2 * h^2)), refused below 1."""
    p, h = check_patch(patch), check_strength(strength, what)
    d = int(np.rint((2 * p + 1) ** 2 * h * h))
    if d < 1:
        raise ValueError(f"{what} = {strength!r} with patch = {p}: the divisor rint((2 P + 1)^2 h^2) is {d}, below 1")
    return d


def check_spatial_options(spatial_denoise, patch, search, strength, chroma_strength, prefix: str = "spatial_"):
    """The spatial_denoise= arguments of upscale_video / VideoUpscaler: None without spatial_denoise= (the options must then be at their
    defaults), else (patch, search, strength, chroma strength) checked; chroma_strength None: the strength.  strength "auto" (upscale_video alone:
    the noise level is measured on the frames, savsr_amd/noise.py) comes back as it is, beside the chroma strength as given."""
    if check_spatial_denoiser(spatial_denoise, f"{prefix}denoise") is None:
        for name, value, default in ((f"{prefix}patch", patch, DEFAULT_PATCH), (f"{prefix}search", search, DEFAULT_SEARCH),
                                     (f"{prefix}strength", strength, DEFAULT_STRENGTH), (f"{prefix}chroma_strength", chroma_strength, None)):
            same = value is None if default is None else (not isinstance(value, bool) and isinstance(value, (int, float, np.integer, np.floating))
                                                          and value == default)
            if not same:
                raise ValueError(f"{name} = {value!r} goes with {prefix}denoise=: without the stage there is nothing to set")
        return None
    p = check_patch(patch, f"{prefix}patch")
    s = check_search(search, f"{prefix}search")
    if isinstance(strength, str) and strength == AUTO:          # found from the frames by the caller; an explicit chroma strength wins
        if chroma_strength is not None:
            divisor(p, chroma_strength, f"{prefix}chroma_strength")
        return p, s, AUTO, None if chroma_strength is None else check_strength(chroma_strength, f"{prefix}chroma_strength")
    h = check_strength(strength, f"{prefix}strength")
    divisor(p, h, f"{prefix}strength")
    ch = h if chroma_strength is None else check_strength(chroma_strength, f"{prefix}chroma_strength")
    divisor(p, ch, f"{prefix}chroma_strength")
    return p, s, h, ch


def _box(d: np.ndarray, p: int) -> np.ndarray:
    """Sums of d over every (2 p + 1)^2 window: an integral image."""
    ii = np.zeros((d.shape[0] + 1, d.shape[1] + 1), dtype=np.int64)
    ii[1:, 1:] = d.cumsum(0).cumsum(1)
    n = 2 * p + 1
    return ii[n:, n:] - ii[:-n, n:] - ii[n:, :-n] + ii[:-n, :-n]


def nlm_matrix(m, depth: int = 8, patch: int = DEFAULT_PATCH, search: int = DEFAULT_SEARCH, divisor: int = 441, return_counts: bool = False):
    """[R, C] integer samples -> [R, C] of the same dtype: the rule of the module's docstring on every sample.  return_counts: (the
    result, counts) with counts = {"k": int64[578], the number of taken candidates per k bucket, zero-weight ones included, entry 577
    holding every k >= 577; "k0_off_centre": the taken candidates with k = 0 other than the centre; "sum_max": the largest numerator}."""
    P, S = check_patch(patch), check_search(search)
    if not _is_int(divisor) or divisor < 1:
        raise ValueError(f"divisor = {divisor!r}: an int >= 1")
    D = int(divisor)
    m = np.asarray(m)
    if m.ndim != 2 or m.dtype.kind not in "iu":
        raise ValueError(f"the matrix must be [R, C] integers, got {m.dtype} {tuple(m.shape)}")
    R, C = m.shape
    if R < 1 or C < 1:
        raise ValueError(f"a matrix of {R} x {C}: R >= 1 and C >= 1")
    if depth not in (8, 10, 12):
        raise ValueError(f"depth = {depth!r}: 8, 10 or 12")
    shift = 2 * (depth - 8)
    v = np.minimum(m.astype(np.int64), (1 << depth) - 1)
    pad = S + P
    vp = np.pad(v, pad, mode="edge")
    table = np.array(WEIGHTS + (0,), dtype=np.int64)
    a = vp[S:S + R + 2 * P, S:S + C + 2 * P]          # the patches' samples around every p
    ys, xs = np.arange(R)[:, None], np.arange(C)[None, :]
    sw = np.zeros((R, C), dtype=np.int64)
    sv = np.zeros((R, C), dtype=np.int64)
    counts = {"k": np.zeros(N_WEIGHTS + 1, dtype=np.int64), "k0_off_centre": 0, "sum_max": 0}
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            b = vp[S + dy:S + dy + R + 2 * P, S + dx:S + dx + C + 2 * P]
            ssd = _box((a - b) ** 2, P)
            k = np.minimum(((ssd >> shift) * 64) // D, N_WEIGHTS)
            taken = (ys + dy >= 0) & (ys + dy < R) & (xs + dx >= 0) & (xs + dx < C)
            w = np.where(taken, table[k], 0)
            sw += w
            sv += w * vp[pad + dy:pad + dy + R, pad + dx:pad + dx + C]
            if return_counts:
                counts["k"] += np.bincount(k[taken], minlength=N_WEIGHTS + 1)
                if dy or dx:
                    counts["k0_off_centre"] += int(np.count_nonzero(taken & (k == 0)))
    counts["sum_max"] = int(sv.max())
    out = ((sv + (sw >> 1)) // sw).astype(m.dtype)
    return (out, counts) if return_counts else out


def _planes(frames: np.ndarray, h: int, w: int, depth: int, layout: str):
    if layout == MONO:
        return [luma_plane(frames, h, w, depth, MONO)]
    return list(split_planes(frames, h, w, depth, layout))


def nlm_frames(frames, pixel_format: str = "rgb", size=None, depth: int = 8, patch: int = DEFAULT_PATCH, search: int = DEFAULT_SEARCH,
               strength=DEFAULT_STRENGTH, chroma_strength=None) -> np.ndarray:
    """N frames -> N filtered frames in the same format: `nlm_matrix` on every plane of every frame.  [N, h, w, c] uint8: every channel as
    a plane of its own with `strength`.  Planar frames (pixel_format "i420", "i422", "i444", "y400" with size=(h, w); [N, frame_bytes]
    uint8, little-endian 16-bit words at depth 10 / 12): the Y plane with `strength`, the chroma planes with `chroma_strength` (None:
    `strength`).  Float frames are refused.  The default strength is a parameter: nothing is validated on footage."""
    p, s = check_patch(patch), check_search(search)
    d = divisor(p, strength)
    cd = d if chroma_strength is None else divisor(p, chroma_strength, "chroma_strength")
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
        n = frames.shape[0]
        parts = []
        for i, pl in enumerate(_planes(frames, h, w, depth, layout)):
            done = np.stack([nlm_matrix(pl[t], depth, p, s, d if i == 0 else cd) for t in range(n)]) if n else pl
            parts.append(np.ascontiguousarray(done.astype(np.uint8 if depth == 8 else "<u2")).reshape(n, -1).view(np.uint8))
        return np.concatenate(parts, 1)
    if depth != 8:
        raise ValueError(f"depth = {depth} goes with pixel_format = 'i420', 'i422', 'i444' or 'y400': packed frames are 8-bit")
    if frames.dtype.kind == "f":
        raise ValueError("float frames have no integer samples to denoise: give [N, h, w, c] uint8 or planar frames (quantise first)")
    if frames.dtype != np.uint8 or frames.ndim != 4:
        raise ValueError(f"frames must be [N, h, w, c] uint8, got {frames.dtype} {tuple(frames.shape)}")
    out = np.empty_like(frames)
    for t in range(frames.shape[0]):
        for ch in range(frames.shape[3]):
            out[t, :, :, ch] = nlm_matrix(frames[t, :, :, ch], 8, p, s, d)
    return out
