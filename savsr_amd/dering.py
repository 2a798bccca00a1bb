"""Deringing in front of the network: the host-side specification (numpy, integers only, no GPU needed).

A coarsely quantised 8 x 8 DCT (MPEG-2: DVD, DVB, DV) puts oscillations around every sharp edge inside the block -- ringing, mosquito
noise -- and a x4 network enlarges them as texture.  No other stage removes them: `deblock=` touches only the samples next to the block
grid, the temporal denoiser leaves static ringing alone by construction, and non-local means finds the ringing repeated along an edge in
every patch and keeps it.  The stage here finds the local edge direction of every 8 x 8 block, smooths along it, and smooths across it
only where the differences are small.  `dering_matrix` is the rule, in integers; csrc/dering.hip equals it bit for bit.  Every frame is
filtered on its own.

The rule, for one matrix m[R, C] of integer samples, R, C >= 1, depth d in {8, 10, 12}, a strength (p, s), ints 0 <= p <= 15 and
0 <= s <= 4, and a damping D, an int 3 <= D <= 6, strength and damping in 8-bit code units at every depth:
  sh = d - 8, top = 2^d - 1, v = min(m, top); at(y, x) = v[clip(y, 0, R - 1)][clip(x, 0, C - 1)]: reads beyond the plane clamp;
  msb(n) = floor(log2 n) for n >= 1.
The plane is cut into 8 x 8 blocks starting at its origin; the last blocks may be partial.  Every block is handled on its own, reads
only v and writes only its own samples inside the plane: no output is ever read, so the order of the blocks cannot matter.

1. Direction.  b[i][j] = (at(8 by + i, 8 bx + j) >> sh) - 128, i, j in 0 .. 7 (a partial block reads clamped copies).  Eight sets of
   line sums, with integer /, each += b[i][j]:
     partial[0][i + j]        partial[1][i + j/2]      partial[2][i]            partial[3][3 + i - j/2]
     partial[4][7 + i - j]    partial[5][3 - i/2 + j]  partial[6][j]            partial[7][i/2 + j]
   and with W = [0, 840, 420, 280, 210, 168, 140, 120, 105]:
     directions 2, 6:        cost[k] = 105 sum_{i<8} partial[k][i]^2
     directions 0, 4:        cost[k] = sum_{i<7} (partial[k][i]^2 + partial[k][14 - i]^2) W[i + 1] + 105 partial[k][7]^2
     directions 1, 3, 5, 7:  cost[k] = 105 sum_{j<5} partial[k][3 + j]^2 + sum_{j<3} (partial[k][j]^2 + partial[k][10 - j]^2) W[2 j + 2]
   dir is the smallest index with the maximal cost; var = (cost[dir] - cost[(dir + 4) & 7]) >> 10.  No cost exceeds 880 803 840 (a
   block of zeros reaches it), so 32-bit signed arithmetic suffices; a constant block has eight equal costs: dir = 0, var = 0.
2. Strengths.  P8 = 0 if var == 0, else (p (4 + i) + 8) >> 4 with i = 0 if var < 64 and min(msb(var >> 6), 12) otherwise;
   P = P8 << sh, S = s << sh, Dd = D + sh.  With P == 0 and S == 0 the block is v, unchanged.
3. Filter.  For every sample x = v[y][c] of the block inside the plane, with
     con(delta, T, q) = sign(delta) min(|delta|, max(0, T - (|delta| >> q)))
   and the two taps (dy, dx) of a direction
     0: (-1, 1) (-2, 2)   1: (0, 1) (-1, 2)   2: (0, 1) (0, 2)   3: (0, 1) (1, 2)
     4: (1, 1) (2, 2)     5: (1, 0) (2, 1)    6: (1, 0) (2, 0)   7: (1, 0) (2, -1)
   primary taps, only if P > 0: weights (4, 2) if P8 is even, (3, 3) if odd, q = max(0, Dd - msb(P)); for k in {0, 1} and both signs,
     t = at(y +- dy_k, c +- dx_k) from dirs[dir], sum += w_k con(t - x, P, q);
   secondary taps, only if S > 0: weights (2, 1), q = max(0, Dd - msb(S)), the same over dirs[(dir + 2) & 7] and dirs[(dir + 6) & 7],
     eight taps in all;
   y' = x + ((8 + sum - (sum < 0)) >> 4), an arithmetic shift, then clamped to [lo, hi], the minimum and maximum of x and every tap read
   in a class whose strength is non-zero.

Packed [N, h, w, c] frames filter every channel as a plane of its own: a tap's dx moves dx pixels, a channel meets only itself.

Interlaced video: `dering_fields` applies `dering_matrix` to the rows 0::2 and to the rows 1::2, each field a plane of its own with its
own 8 x 8 blocks and clamp, so that no filter mixes two moments.  A field with no rows (R = 1) is legal.

What follows from the rule (tests/test_dering.py holds it): a constant plane comes back unchanged; (0, 0) is the identity on v; every
output lies within the minimum and maximum of x and its taps; no sample moves by more than (12 (P + S) + 8) >> 4 with P8 <= 15 (each
class's weights sum to 12 and |con| <= its strength); a block's output depends on nothing outside the block plus a ring of 2 samples, so
splitting a plane at a multiple of 8 changes only samples within 2 of the cut.  Equivariance under flips is not promised: the tie rule
and the partial blocks break it.

Planar frames ("i420", "i422", "i444", "y400" at 8, 10 or 12 bits) filter every plane by the same rule in the plane's own samples: Y with
`strength`, chroma with `chroma_strength` (None: the strength).  Float frames are refused.

How far AV1 is followed: the idea is that of AV1's constrained directional enhancement filter (CDEF) -- a direction search per 8 x 8
block on line sums, a primary filter along the direction and a secondary one across it, both constrained by a strength and a damping, the
primary strength scaled by the block's directional variance.  The definition is this project's: the clamped reads at the plane's end in
place of skipped taps, the grid at the plane's origin, partial blocks, the field-wise form, one strength per video where a bitstream
signals one per 64 x 64 block, chroma with a direction of its own, and the 8-bit scale of strength and damping at every depth.  Neither
libaom nor ffmpeg is available where this was written: nothing here is pinned to libaom's or ffmpeg's output.  The defaults are
parameters; nothing is validated on footage.  The 8 x 8 analysis grid starts at the plane's origin and does not follow `deblock_origin`;
the stage also smooths fine noise.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from .frames import check_pixel_format, layout_of
from .yuv import MONO, check_depth, frame_bytes, layout_name, luma_plane, split_planes

DERINGERS = ("cdef",)
DEFAULT_STRENGTH = (4, 2)            # (primary, secondary) in 8-bit code units; parameters: nothing is validated on footage
DEFAULT_DAMPING = 5
MAX_PRIMARY, MAX_SECONDARY = 15, 4
MIN_DAMPING, MAX_DAMPING = 3, 6
BLOCK = 8

COST_WEIGHTS = (0, 840, 420, 280, 210, 168, 140, 120, 105)
# the two taps (dy, dx) of every direction
DIRECTIONS = (((-1, 1), (-2, 2)), ((0, 1), (-1, 2)), ((0, 1), (0, 2)), ((0, 1), (1, 2)),
              ((1, 1), (2, 2)), ((1, 0), (2, 1)), ((1, 0), (2, 0)), ((1, 0), (2, -1)))


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_deringer(dering, what: str = "dering") -> Optional[str]:
    """dering is None or one of DERINGERS."""
    if dering is None:
        return None
    if not isinstance(dering, str) or dering not in DERINGERS:
        raise ValueError(f"{what} = {dering!r}: None or one of {', '.join(DERINGERS)}")
    return dering


def check_strength(strength, what: str = "strength") -> Tuple[int, int]:
    """(p, s): the primary strength, an int in 0 .. 15, and the secondary one, an int in 0 .. 4, in 8-bit code units at every depth."""
    ok = (isinstance(strength, (tuple, list)) and len(strength) == 2 and all(_is_int(v) for v in strength)
          and 0 <= strength[0] <= MAX_PRIMARY and 0 <= strength[1] <= MAX_SECONDARY)
    if not ok:
        raise ValueError(f"{what} = {strength!r}: two ints (p, s), 0 <= p <= {MAX_PRIMARY} and 0 <= s <= {MAX_SECONDARY}, in 8-bit code units at "
                         f"every depth (p bounds the smoothing along a block's direction, s the smoothing across it)")
    return int(strength[0]), int(strength[1])


def check_damping(damping, what: str = "damping") -> int:
    """An int in 3 .. 6: a tap whose difference reaches strength << (damping - msb(strength)) is left out."""
    if not _is_int(damping) or not MIN_DAMPING <= damping <= MAX_DAMPING:
        raise ValueError(f"{what} = {damping!r}: an int in {MIN_DAMPING} .. {MAX_DAMPING}, in 8-bit code units at every depth (larger: taps "
                         f"with larger differences still count)")
    return int(damping)


def _same(value, default) -> bool:
    if default is None:
        return value is None
    if isinstance(default, tuple):
        return isinstance(value, (tuple, list)) and len(value) == len(default) and all(_is_int(v) and v == d for v, d in zip(value, default))
    return _is_int(value) and value == default


def check_dering_options(dering, strength, chroma_strength, damping, prefix: str = "dering_"):
    """The dering= arguments of upscale_video / VideoUpscaler: None without dering= (the options must then be at their defaults), else
    (strength, chroma strength, damping) checked; chroma_strength None: the strength."""
    stage = prefix.rstrip("_") or "dering"
    if check_deringer(dering, stage) is None:
        for name, value, default in ((f"{prefix}strength", strength, DEFAULT_STRENGTH), (f"{prefix}chroma_strength", chroma_strength, None),
                                     (f"{prefix}damping", damping, DEFAULT_DAMPING)):
            if not _same(value, default):
                raise ValueError(f"{name} = {value!r} goes with {stage}=: without the stage there is nothing to set")
        return None
    s = check_strength(strength, f"{prefix}strength")
    cs = s if chroma_strength is None else check_strength(chroma_strength, f"{prefix}chroma_strength")
    return s, cs, check_damping(damping, f"{prefix}damping")


def _msb(a: np.ndarray) -> np.ndarray:
    """floor(log2 a) of every a >= 1, in integers (0 where a < 1)."""
    r = np.zeros_like(a)
    for k in range(1, 32):
        r += (a >> k) > 0
    return r


def _line(k: int, i: int, j: int) -> int:
    return (i + j, i + j // 2, i, 3 + i - j // 2, 7 + i - j, 3 - i // 2 + j, j, i // 2 + j)[k]


def block_directions(v: np.ndarray, depth: int = 8):
    """(dir, var), int64 [ceil(R / 8), ceil(C / 8)]: step 1 of the rule for every block of v[R, C] (int64, already min(m, top))."""
    R, C = v.shape
    nby, nbx = -(-R // BLOCK), -(-C // BLOCK)
    ys, xs = np.minimum(np.arange(nby * BLOCK), R - 1), np.minimum(np.arange(nbx * BLOCK), C - 1)
    b = ((v[ys][:, xs] >> (depth - 8)) - 128).reshape(nby, BLOCK, nbx, BLOCK)
    partial = np.zeros((8, 15, nby, nbx), np.int64)
    for i in range(BLOCK):
        for j in range(BLOCK):
            for k in range(8):
                partial[k, _line(k, i, j)] += b[:, i, :, j]
    sq, W = partial * partial, COST_WEIGHTS
    cost = np.zeros((8, nby, nbx), np.int64)
    for k in (2, 6):
        cost[k] = 105 * sq[k, :8].sum(0)
    for k in (0, 4):
        cost[k] = sum((sq[k, i] + sq[k, 14 - i]) * W[i + 1] for i in range(7)) + 105 * sq[k, 7]
    for k in (1, 3, 5, 7):
        cost[k] = 105 * sq[k, 3:8].sum(0) + sum((sq[k, j] + sq[k, 10 - j]) * W[2 * j + 2] for j in range(3))
    d = np.argmax(cost, 0)          # (the first of equal maxima: the smallest index)
    best = np.take_along_axis(cost, d[None], 0)[0]
    across = np.take_along_axis(cost, ((d + 4) & 7)[None], 0)[0]
    return d.astype(np.int64), (best - across) >> 10


def primary8(var: np.ndarray, p: int) -> np.ndarray:
    """P8 of step 2 for every block."""
    i = np.where(var < 64, 0, np.minimum(_msb(var >> 6), 12))
    return np.where(var == 0, 0, (p * (4 + i) + 8) >> 4)


def _con(delta: np.ndarray, T, q) -> np.ndarray:
    ad = np.abs(delta)
    return np.sign(delta) * np.minimum(ad, np.maximum(0, T - (ad >> q)))


def dering_matrix(m, depth: int = 8, strength=DEFAULT_STRENGTH, damping: int = DEFAULT_DAMPING, return_counts: bool = False):
    """[R, C] integer samples -> [R, C] of the same dtype: the rule of the module's docstring.  return_counts: (the result, counts) with
    counts of blocks: "flat" (var == 0), "var_low" (0 < var < 64), "var_high" (var >= 64), "even_taps" (P > 0, weights (4, 2)),
    "odd_taps" (P > 0, weights (3, 3)), and "changed", the samples that differ from v."""
    p, s = check_strength(strength)
    D = check_damping(damping)
    m = np.asarray(m)
    if m.ndim != 2 or m.dtype.kind not in "iu":
        raise ValueError(f"the matrix must be [R, C] integers, got {m.dtype} {tuple(m.shape)}")
    R, C = m.shape
    if R < 1 or C < 1:
        raise ValueError(f"a matrix of {R} x {C}: R >= 1 and C >= 1")
    if depth not in (8, 10, 12):
        raise ValueError(f"depth = {depth!r}: 8, 10 or 12")
    sh, top = depth - 8, (1 << depth) - 1
    v = np.minimum(m.astype(np.int64), top)
    d_b, var_b = block_directions(v, depth)
    P8_b = primary8(var_b, p)
    grow = lambda a: np.repeat(np.repeat(a, BLOCK, 0), BLOCK, 1)[:R, :C]          # noqa: E731  (a block's value at each of its samples)
    dirs, P8 = grow(d_b), grow(P8_b)
    P, S, Dd = P8 << sh, s << sh, D + sh
    vp = np.pad(v, 2, mode="edge")          # (no tap reaches beyond 2: the padding is the clamp)
    Y, X = np.mgrid[0:R, 0:C]
    table = np.array(DIRECTIONS, np.int64)          # [8, 2, 2]
    total = np.zeros_like(v)
    lo, hi = v.copy(), v.copy()

    def taps(direction, weights, T, q, on):
        nonlocal total, lo, hi
        for k in (0, 1):
            dy, dx = table[direction, k, 0], table[direction, k, 1]
            for sign in (1, -1):
                t = vp[Y + 2 + sign * dy, X + 2 + sign * dx]
                total = total + np.where(on, weights[k] * _con(t - v, T, q), 0)
                lo, hi = np.where(on, np.minimum(lo, t), lo), np.where(on, np.maximum(hi, t), hi)

    if p > 0:
        odd = (P8 & 1) == 1
        qp = np.maximum(0, Dd - _msb(np.maximum(P, 1)))
        taps(dirs, (np.where(odd, 3, 4), np.where(odd, 3, 2)), P, qp, P > 0)
    if S > 0:
        qs = max(0, Dd - (int(S).bit_length() - 1))
        taps((dirs + 2) & 7, (2, 1), S, qs, True)
        taps((dirs + 6) & 7, (2, 1), S, qs, True)
    res = np.clip(v + ((8 + total - (total < 0)) >> 4), lo, hi)
    out = res.astype(m.dtype)
    if not return_counts:
        return out
    counts = {"flat": int(np.count_nonzero(var_b == 0)), "var_low": int(np.count_nonzero((var_b > 0) & (var_b < 64))),
              "var_high": int(np.count_nonzero(var_b >= 64)), "even_taps": int(np.count_nonzero((P8_b > 0) & (P8_b % 2 == 0))),
              "odd_taps": int(np.count_nonzero(P8_b % 2 == 1)), "changed": int(np.count_nonzero(res != v))}
    return out, counts


def dering_fields(m, depth: int = 8, strength=DEFAULT_STRENGTH, damping: int = DEFAULT_DAMPING) -> np.ndarray:
    """[R, C] integer samples of an interlaced frame -> [R, C]: `dering_matrix` on the rows 0::2 and on the rows 1::2, each field a plane
    of its own with its own blocks and clamp.  R = 1 (an empty second field) is legal."""
    m = np.asarray(m)
    if m.ndim != 2 or m.dtype.kind not in "iu":
        raise ValueError(f"the matrix must be [R, C] integers, got {m.dtype} {tuple(m.shape)}")
    out = np.empty_like(m)
    for par in (0, 1):
        if m[par::2].shape[0]:
            out[par::2] = dering_matrix(m[par::2], depth, strength, damping)
    return out


def dering_plane(m, depth: int = 8, strength=DEFAULT_STRENGTH, damping: int = DEFAULT_DAMPING, interlaced: bool = False) -> np.ndarray:
    """One plane as the stage filters it: `dering_fields` for interlaced video, else `dering_matrix`."""
    return dering_fields(m, depth, strength, damping) if interlaced else dering_matrix(m, depth, strength, damping)


def _planes(frames: np.ndarray, h: int, w: int, depth: int, layout: str):
    if layout == MONO:
        return [luma_plane(frames, h, w, depth, MONO)]
    return list(split_planes(frames, h, w, depth, layout))


def dering_frames(frames, pixel_format: str = "rgb", size=None, depth: int = 8, strength=DEFAULT_STRENGTH, chroma_strength=None,
                  damping: int = DEFAULT_DAMPING, interlaced: bool = False) -> np.ndarray:
    """N frames -> N filtered frames in the same format: `dering_plane` on every plane of every frame.  [N, h, w, c] uint8: every channel
    as a plane of its own with `strength`.  Planar frames (pixel_format "i420", "i422", "i444", "y400" with size=(h, w); [N, frame_bytes]
    uint8, little-endian 16-bit words at depth 10 / 12): the Y plane with `strength`, the chroma planes with `chroma_strength` (None:
    `strength`).  interlaced: every plane field by field.  Float frames are refused.  The defaults are parameters: nothing is validated
    on footage."""
    s = check_strength(strength)
    cs = s if chroma_strength is None else check_strength(chroma_strength, "chroma_strength")
    damping = check_damping(damping)
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
            done = np.stack([dering_plane(pl[t], depth, s if i == 0 else cs, damping, interlaced) for t in range(n)]) if n else pl
            parts.append(np.ascontiguousarray(done.astype(np.uint8 if depth == 8 else "<u2")).reshape(n, -1).view(np.uint8))
        return np.concatenate(parts, 1)
    if depth != 8:
        raise ValueError(f"depth = {depth} goes with pixel_format = 'i420', 'i422', 'i444' or 'y400': packed frames are 8-bit")
    if frames.dtype.kind == "f":
        raise ValueError("float frames have no integer samples to dering: give [N, h, w, c] uint8 or planar frames (quantise first)")
    if frames.dtype != np.uint8 or frames.ndim != 4:
        raise ValueError(f"frames must be [N, h, w, c] uint8, got {frames.dtype} {tuple(frames.shape)}")
    out = np.empty_like(frames)
    for t in range(frames.shape[0]):
        for ch in range(frames.shape[3]):
            out[t, :, :, ch] = dering_plane(frames[t, :, :, ch], 8, s, damping, interlaced)
    return out
