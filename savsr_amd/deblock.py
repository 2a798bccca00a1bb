"""Deblocking in front of the network: the host-side specification (numpy, integers only, no GPU needed).

MPEG-2 (DVD, DVB, DV) has no in-loop filter, so every MPEG-2 stream and many low-bitrate H.264 rips carry 8 x 8 block edges; a x4 network
enlarges a 2 .. 6 code step along a block border as a sharp edge on a 32-pixel grid.  Neither denoiser removes it: the temporal one leaves
a static grid alone by construction, and non-local means finds the step repeated in every patch along the border and keeps it.  The stage
here smooths the samples next to the block grid where the step across it is small and both sides are flat.  `deblock_matrix` is the rule,
in integers; csrc/deblock.hip equals it bit for bit.  Every frame is filtered on its own.

The rule, for one matrix m[R, C] of integer samples, depth d in {8, 10, 12}, blocks block_y in {2, 4, 8, 16} and block_x in {4, 8, 16},
a mode ("weak" or "strong") and thresholds thr = (a, b), ints in 0 .. 255, in 8-bit code units at every depth:
  v = min(m, 2^d - 1); every output is computed from v, the samples no filter touches included;  A = a << (d - 8), Bt = b << (d - 8);
  pass X filters across the vertical edges e = ox + k block_x, 1 <= e <= C - 1, every row on its own;
  pass Y then filters across the horizontal edges e = oy + k block_y, 1 <= e <= R - 1, every column on its own, reading pass X's result.
(oy, ox), 0 <= o < block in its direction, is the grid's origin, (0, 0) by default: a video whose bars or overscan were cropped by c
samples before it arrived has its edges at (-c) mod block.  For one line and one edge the samples are P2 P1 P0 | Q0 Q1 Q2, P0 at e - 1
and Q0 at e.  Coordinates beyond the plane clamp to it for reading (at origin 0 only the Q side can lie beyond it: e >= 4; with an
origin the P side can: e < 3); positions beyond the plane are not written.  The origin adds nothing to the rule: the result at (oy, ox)
is the result at (0, 0) on the plane padded by (block_y - oy) % block_y rows above and (block_x - ox) % block_x columns to the left
with copies of its first row and column, without the padding (tests/test_grid.py holds it).  With delta = Q0 - P0 and
t(n) = sign(delta) (|delta| >> log2 n) -- truncation toward zero --
  weak    applies iff |delta| < A, |P0 - P1| < Bt and |Q0 - Q1| < Bt:
          P1 += t(8), P0 += t(2), Q0 -= t(2), Q1 -= t(8);
  strong  needs these and |P1 - P2| < Bt and |Q1 - Q2| < Bt (where one fails nothing is filtered: there is no fall-back to weak):
          P2 += t(8), P1 += t(4), P0 += t(2), Q0 -= t(2), Q1 -= t(4), Q2 -= t(8);
and every written sample is clamped to [0, 2^d - 1].  All the reads of a line are taken before its writes.

A direction whose block is below 8 takes the weak filter even under mode "strong".  That holds by definition, and it is what makes a pass
well defined: weak reads and writes 2 samples a side and 2 + 2 <= 4, strong 3 a side and 3 + 3 <= 8, so with the filter a direction is
allowed the samples of two edges of one pass never overlap -- an edge's six (or four) samples end before the next edge's begin, and the
clamped copies beyond the plane belong to the last edge alone -- and the order in which a pass takes its edges cannot matter.  The two
passes do not commute: a sample near a corner of the grid is moved by both, and pass Y's conditions read what pass X wrote.

block_y = 2 arises only from field-wise filtering at block 4 (below): a 2-row block has no interior, both of its rows would belong to two
edges at once, so pass Y is left out and the rule is pass X alone.

Interlaced video: `deblock_fields(m, depth, block, mode, thr)` applies `deblock_matrix` with (block_y, block_x) = (block // 2, block) to
the rows 0::2 and to the rows 1::2, each field a plane of its own, so that no filter mixes two moments.  A field with no rows (R = 1) is
legal.  At block 8 the fields' block_y is 4, so the vertical direction takes the weak filter; at block 4 there is no pass Y.  The origin's
oy must be even there (an odd one swaps the fields' parity) and each field takes (oy // 2, ox).

What follows from the rule (tests/test_deblock.py holds it): a constant plane comes back unchanged; a = 0 is the identity on v; one pass
moves no sample by more than (A - 1) // 2 (|delta| <= A - 1 and the largest step is t(2)), so the two passes together move none by more
than 2 ((A - 1) // 2), which a corner of the grid reaches (four flat blocks of 0, 20 / 20, 40 at a = 25: the corner sample goes 0 -> 10
-> 20); where no write is clamped or dropped at the plane's end -- both dimensions multiples of their blocks is enough for the second --
the plane's sum is conserved exactly (every +t(n) has its -t(n)); the rule is equivariant under up/down and left/right flips when the
flipped dimension is a multiple of its block (P and Q change places, delta changes sign, and truncation toward zero is symmetric); it is
not equivariant under transposition, because the passes have an order.

Planar frames ("i420", "i422", "i444", "y400" at 8, 10 or 12 bits) filter every plane with the same `block` in the plane's own samples:
Y with `strength`, chroma with `chroma_strength` (None: the strength).  [N, h, w, c] uint8 frames filter every channel as a plane of its
own: a channel only meets itself.  Float frames are refused.

How far ffmpeg is followed: the idea of ffmpeg's `deblock` filter is kept -- a weak and a strong filter across the edges of a fixed grid,
gated by one threshold on the step and one on the flatness of either side, corrections of delta / 2, / 4 and / 8 -- and its default
thresholds (0.098 and 0.05 of full scale: 25 and 13 codes).  The integer form, the order of the passes with the second reading the
first, truncation toward zero, the clamped reads and dropped writes at the plane's end, the weak filter below block 8, the field-wise
form and the thresholds' 8-bit scale at every depth are this project's.  ffmpeg is not available where this was written: nothing here is
pinned to its output.  The defaults are parameters; nothing is validated on footage.  There is one grid (block size and origin; savsr_amd/grid.py
finds them from the frames), and one strength per video, and no adaptation to the stream's quantiser, which a tensor does not carry.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from .frames import check_pixel_format, layout_of
from .yuv import MONO, check_depth, frame_bytes, layout_name, luma_plane, split_planes

DEBLOCKERS = ("weak", "strong")
BLOCKS = (4, 8, 16)
DEFAULT_BLOCK = 8
DEFAULT_STRENGTH = (25, 13)          # ffmpeg deblock's 0.098 / 0.05 in 8-bit codes; parameters: nothing is validated on footage
MAX_THRESHOLD = 255


def check_deblocker(deblock, what: str = "deblock") -> Optional[str]:
    """deblock is None or one of DEBLOCKERS."""
    if deblock is None:
        return None
    if not isinstance(deblock, str) or deblock not in DEBLOCKERS:
        raise ValueError(f"{what} = {deblock!r}: None or one of {', '.join(DEBLOCKERS)}")
    return deblock


def check_mode(mode, what: str = "mode") -> str:
    """mode is one of DEBLOCKERS."""
    if not isinstance(mode, str) or mode not in DEBLOCKERS:
        raise ValueError(f"{what} = {mode!r}: one of {', '.join(DEBLOCKERS)}")
    return mode


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_block(block, what: str = "block") -> int:
    """The block is 4, 8 or 16 samples, in every plane's own samples."""
    if not _is_int(block) or block not in BLOCKS:
        raise ValueError(f"{what} = {block!r}: 4, 8 or 16 (the coded block's size in samples; the grid starts at the frame's origin)")
    return int(block)


def check_strength(strength, what: str = "strength") -> Tuple[int, int]:
    """(a, b): two ints in 0 .. 255, in 8-bit code units at every depth."""
    ok = isinstance(strength, (tuple, list)) and len(strength) == 2 and all(_is_int(v) and 0 <= v <= MAX_THRESHOLD for v in strength)
    if not ok:
        raise ValueError(f"{what} = {strength!r}: two ints (a, b) in 0 .. {MAX_THRESHOLD}, in 8-bit code units at every depth (an edge is "
                         f"filtered where its step is below a and the steps beside it are below b)")
    return int(strength[0]), int(strength[1])


def _pair(value) -> bool:
    return isinstance(value, (tuple, list)) and len(value) == 2 and all(_is_int(v) for v in value)


def check_origin(origin, block: int, interlaced: bool = False, what: str = "origin") -> Tuple[int, int]:
    """(oy, ox): two ints in 0 .. block - 1, the grid's first edges in the plane's samples; oy even where the plane is filtered field by
    field (an odd one would swap the fields' parity)."""
    if not _pair(origin) or not all(0 <= v < block for v in origin):
        raise ValueError(f"{what} = {origin!r}: two ints (oy, ox) in 0 .. {block - 1} (the grid's first edges in the plane's samples, below "
                         f"the block {block})")
    if interlaced and origin[0] % 2:
        raise ValueError(f"{what} = {origin!r}: oy must be even on a field-wise run (an odd origin swaps the fields' parity; each field takes "
                         f"(oy // 2, ox))")
    return int(origin[0]), int(origin[1])


SUBSAMPLED = ("420", "422")          # the layouts whose chroma planes are smaller than the Y plane


def check_origins(origin, chroma_origin, block: int, interlaced: bool = False, layout: Optional[str] = None, prefix: str = ""):
    """(origin, chroma origin) checked.  chroma_origin None means the origin, which a subsampled layout refuses unless that is (0, 0): a
    crop of c luma samples moves the luma grid to (-c) mod block and the chroma grid to (-c / 2) mod block, so neither follows from
    the other."""
    o = check_origin(origin, block, interlaced, f"{prefix}origin")
    if chroma_origin is None:
        if o != (0, 0) and layout in SUBSAMPLED:
            raise ValueError(f"{prefix}origin = {o!r} on 4:{layout[1]}:{layout[2]} frames needs {prefix}chroma_origin=: the chroma grid of a cropped video "
                             f"does not follow from the luma's (a crop of c moves them to (-c) mod {block} and (-c / 2) mod {block})")
        return o, o
    return o, check_origin(chroma_origin, block, interlaced, f"{prefix}chroma_origin")


def _same(value, default) -> bool:
    if default is None:
        return value is None
    if isinstance(default, tuple):
        return isinstance(value, (tuple, list)) and len(value) == len(default) and all(_is_int(v) and v == d for v, d in zip(value, default))
    if isinstance(default, str):
        return value == default
    return _is_int(value) and value == default


def check_deblock_options(deblock, block, strength, chroma_strength, prefix: str = "deblock_", origin=(0, 0), chroma_origin=None, grid=None):
    """The deblock= arguments of upscale_video / VideoUpscaler: None without deblock= (the options must then be at their defaults), else
    (block, mode, strength, chroma strength) checked; chroma_strength None: the strength.  origin, chroma_origin and grid (None or
    "auto") are checked here as far as they can be without the frames (`check_grid_options` has the rest)."""
    stage = prefix.rstrip("_") or "deblock"
    if grid is not None and grid != "auto":
        raise ValueError(f"{prefix}grid = {grid!r}: None or 'auto'")
    if check_deblocker(deblock, stage) is None:
        for name, value, default in ((f"{prefix}block", block, DEFAULT_BLOCK), (f"{prefix}strength", strength, DEFAULT_STRENGTH),
                                     (f"{prefix}chroma_strength", chroma_strength, None), (f"{prefix}origin", origin, (0, 0)),
                                     (f"{prefix}chroma_origin", chroma_origin, None), (f"{prefix}grid", grid, None)):
            if not _same(value, default):
                raise ValueError(f"{name} = {value!r} goes with {stage}=: without the stage there is nothing to set")
        return None
    if grid == "auto":
        for name, value, default in ((f"{prefix}block", block, DEFAULT_BLOCK), (f"{prefix}origin", origin, (0, 0)),
                                     (f"{prefix}chroma_origin", chroma_origin, None)):
            if not _same(value, default):
                raise ValueError(f"{name} = {value!r} together with {prefix}grid = 'auto': the detector answers it; give one or the other")
    b = check_block(block, f"{prefix}block")
    s = check_strength(strength, f"{prefix}strength")
    cs = s if chroma_strength is None else check_strength(chroma_strength, f"{prefix}chroma_strength")
    return b, deblock, s, cs


def _pass(v: np.ndarray, block: int, strong: bool, A: int, Bt: int, top: int, counts: Optional[dict], origin: int = 0) -> np.ndarray:
    """One pass across the edges e = origin + k block, 1 <= e <= C - 1, along the last axis of v (int64, already min(m, top))."""
    C = v.shape[1]
    out = v.copy()
    es = np.arange(origin if origin >= 1 else block, C, block)
    if not es.size:
        return out
    P2, P1, P0, Q0, Q1, Q2 = (v[:, np.clip(es + o, 0, C - 1)] for o in (-3, -2, -1, 0, 1, 2))
    d = Q0 - P0
    ad, sg = np.abs(d), np.sign(d)
    flat = (np.abs(P0 - P1) < Bt) & (np.abs(Q0 - Q1) < Bt)
    if strong:
        flat &= (np.abs(P1 - P2) < Bt) & (np.abs(Q1 - Q2) < Bt)
        writes = ((-3, P2 + sg * (ad >> 3)), (-2, P1 + sg * (ad >> 2)), (-1, P0 + sg * (ad >> 1)),
                  (0, Q0 - sg * (ad >> 1)), (1, Q1 - sg * (ad >> 2)), (2, Q2 - sg * (ad >> 3)))
    else:
        writes = ((-2, P1 + sg * (ad >> 3)), (-1, P0 + sg * (ad >> 1)), (0, Q0 - sg * (ad >> 1)), (1, Q1 - sg * (ad >> 3)))
    ok = (ad < A) & flat
    if counts is not None:
        counts["filtered"] += int(np.count_nonzero(ok))
        counts["refused_a"] += int(np.count_nonzero(ad >= A))
        counts["refused_b"] += int(np.count_nonzero((ad < A) & ~flat))
    for o, val in writes:
        cols = es + o
        keep = (cols >= 0) & (cols <= C - 1)
        if counts is not None:
            counts["clamped"] += int(np.count_nonzero(ok[:, keep] & ((val[:, keep] < 0) | (val[:, keep] > top))))
            counts["dropped"] += int(np.count_nonzero(ok[:, ~keep]))
        out[:, cols[keep]] = np.where(ok[:, keep], np.clip(val[:, keep], 0, top), v[:, cols[keep]])
    return out


def deblock_matrix(m, depth: int = 8, block_y: int = 8, block_x: int = 8, mode: str = "weak", thr=DEFAULT_STRENGTH, return_counts: bool = False,
                   origin_y: int = 0, origin_x: int = 0):
    """[R, C] integer samples -> [R, C] of the same dtype: the rule of the module's docstring.  return_counts: (the result, counts) with
    counts = {"filtered", "refused_a" (|delta| >= A), "refused_b" (a flatness condition alone), the line-edge pairs of both passes;
    "clamped", the writes clamped at 0 or 2^d - 1; "dropped", the writes that fell beyond the plane}.  origin_y, origin_x: the grid's
    origin, 0 <= o < block in its direction: the edges are e = o + k block."""
    mode = check_mode(mode)
    a, b = check_strength(thr, "thr")
    if not _is_int(block_x) or block_x not in BLOCKS:
        raise ValueError(f"block_x = {block_x!r}: 4, 8 or 16")
    if not _is_int(block_y) or block_y not in (2,) + BLOCKS:
        raise ValueError(f"block_y = {block_y!r}: 2 (the fields of block 4: no pass Y), 4, 8 or 16")
    for name, o, blk in (("origin_y", origin_y, block_y), ("origin_x", origin_x, block_x)):
        if not _is_int(o) or not 0 <= o < blk:
            raise ValueError(f"{name} = {o!r}: an int in 0 .. {blk - 1} (the grid's first edge; below the block {blk} of its direction)")
    m = np.asarray(m)
    if m.ndim != 2 or m.dtype.kind not in "iu":
        raise ValueError(f"the matrix must be [R, C] integers, got {m.dtype} {tuple(m.shape)}")
    R, C = m.shape
    if R < 1 or C < 1:
        raise ValueError(f"a matrix of {R} x {C}: R >= 1 and C >= 1")
    if depth not in (8, 10, 12):
        raise ValueError(f"depth = {depth!r}: 8, 10 or 12")
    top = (1 << depth) - 1
    A, Bt = a << (depth - 8), b << (depth - 8)
    counts = {"filtered": 0, "refused_a": 0, "refused_b": 0, "clamped": 0, "dropped": 0} if return_counts else None
    v = np.minimum(m.astype(np.int64), top)
    v = _pass(v, int(block_x), mode == "strong" and block_x >= 8, A, Bt, top, counts, int(origin_x))
    if block_y >= 4:          # (a 2-row block has no interior: no pass Y)
        v = _pass(v.T, int(block_y), mode == "strong" and block_y >= 8, A, Bt, top, counts, int(origin_y)).T
    out = v.astype(m.dtype)
    return (out, counts) if return_counts else out


def deblock_fields(m, depth: int = 8, block: int = DEFAULT_BLOCK, mode: str = "weak", thr=DEFAULT_STRENGTH, origin=(0, 0)) -> np.ndarray:
    """[R, C] integer samples of an interlaced frame -> [R, C]: `deblock_matrix` with (block_y, block_x) = (block // 2, block) on the rows
    0::2 and on the rows 1::2, each field a plane of its own.  R = 1 (an empty second field) is legal.  origin = (oy, ox) in frame
    samples, oy even (an odd one would swap the fields' parity): each field takes the origin (oy // 2, ox)."""
    block = check_block(block)
    oy, ox = check_origin(origin, block, True)
    m = np.asarray(m)
    if m.ndim != 2 or m.dtype.kind not in "iu":
        raise ValueError(f"the matrix must be [R, C] integers, got {m.dtype} {tuple(m.shape)}")
    out = np.empty_like(m)
    for p in (0, 1):
        if m[p::2].shape[0]:
            out[p::2] = deblock_matrix(m[p::2], depth, block // 2, block, mode, thr, origin_y=oy // 2, origin_x=ox)
    return out


def deblock_plane(m, depth: int = 8, block: int = DEFAULT_BLOCK, mode: str = "weak", thr=DEFAULT_STRENGTH, interlaced: bool = False,
                  origin=(0, 0)) -> np.ndarray:
    """One plane as the stage filters it: `deblock_fields` for interlaced video, else `deblock_matrix` with the block both ways; the
    grid's origin = (oy, ox) in the plane's samples."""
    block = check_block(block)
    oy, ox = check_origin(origin, block, interlaced)
    if interlaced:
        return deblock_fields(m, depth, block, mode, thr, (oy, ox))
    return deblock_matrix(m, depth, block, block, mode, thr, origin_y=oy, origin_x=ox)


def _planes(frames: np.ndarray, h: int, w: int, depth: int, layout: str):
    if layout == MONO:
        return [luma_plane(frames, h, w, depth, MONO)]
    return list(split_planes(frames, h, w, depth, layout))


def deblock_frames(frames, pixel_format: str = "rgb", size=None, depth: int = 8, block: int = DEFAULT_BLOCK, mode: str = "weak",
                   strength=DEFAULT_STRENGTH, chroma_strength=None, interlaced: bool = False, origin=(0, 0), chroma_origin=None) -> np.ndarray:
    """N frames -> N filtered frames in the same format: `deblock_plane` on every plane of every frame.  [N, h, w, c] uint8: every channel
    as a plane of its own with `strength`.  Planar frames (pixel_format "i420", "i422", "i444", "y400" with size=(h, w); [N, frame_bytes]
    uint8, little-endian 16-bit words at depth 10 / 12): the Y plane with `strength`, the chroma planes with `chroma_strength` (None:
    `strength`), the same `block` in every plane's own samples.  interlaced: every plane field by field.  Float frames are refused.  The
    defaults are parameters: nothing is validated on footage.  origin = (oy, ox): the grid's origin in the Y plane (in every channel of
    packed frames); chroma_origin: that of the Cb / Cr planes in chroma samples (None: the origin, which subsampled layouts refuse
    when it is not (0, 0))."""
    block, mode = check_block(block), check_mode(mode)
    s = check_strength(strength)
    cs = s if chroma_strength is None else check_strength(chroma_strength, "chroma_strength")
    hw = check_pixel_format(pixel_format, size)
    o, co = check_origins(origin, chroma_origin, block, interlaced, layout_of(pixel_format) if hw else None)
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
            done = np.stack([deblock_plane(pl[t], depth, block, mode, s if i == 0 else cs, interlaced, o if i == 0 else co) for t in range(n)]) if n else pl
            parts.append(np.ascontiguousarray(done.astype(np.uint8 if depth == 8 else "<u2")).reshape(n, -1).view(np.uint8))
        return np.concatenate(parts, 1)
    if depth != 8:
        raise ValueError(f"depth = {depth} goes with pixel_format = 'i420', 'i422', 'i444' or 'y400': packed frames are 8-bit")
    if frames.dtype.kind == "f":
        raise ValueError("float frames have no integer samples to deblock: give [N, h, w, c] uint8 or planar frames (quantise first)")
    if frames.dtype != np.uint8 or frames.ndim != 4:
        raise ValueError(f"frames must be [N, h, w, c] uint8, got {frames.dtype} {tuple(frames.shape)}")
    out = np.empty_like(frames)
    for t in range(frames.shape[0]):
        for ch in range(frames.shape[3]):
            out[t, :, :, ch] = deblock_plane(frames[t, :, :, ch], 8, block, mode, s, interlaced, o)
    return out
