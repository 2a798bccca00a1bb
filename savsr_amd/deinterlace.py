"""Interlaced video: the motion-adaptive deinterlacer's host-side specification (numpy, integers only, no GPU needed).

An interlaced frame weaves two fields taken half a frame period apart.  A video of N interlaced frames becomes 2N progressive frames of
the same size and sample format: output frame 2n + f takes field f of source frame n (f = 0: the earlier field in time).  Its kept rows
are the rows y with y % 2 == p, p = f for "tff" (top field first) and 1 - f for "bff"; they are copied.  The other rows are interpolated
by the rule of ffmpeg's `yadif` filter with its spatial-interlacing check on and every frame treated as interlaced (`deinterlace_matrix`
is that rule, sample by sample, in integers; csrc/deinterlace.hip equals it bit for bit).  `upscale_video(v, fields=o, ...)` is, bit for
bit, `upscale_video(deinterlace(v, o, ...), ...)`: the deinterlacer comes before anything else looks at the video.

The rule works on one matrix of R rows x C samples with a pixel step s (1 for a plane, c for the h x (w * c) byte matrix of packed
frames, so that a channel only meets itself).  With cur = frame n, prev = frame max(n - 1, 0), next = frame min(n + 1, N - 1), p2 / n2 =
prev / cur for f = 0 and cur / next for f = 1, up = y - 1 (y + 1 where y = 0) and dn = y + 1 (y - 1 where y = R - 1), an interpolated
sample (y, x) is the spatial prediction -- (c + e) >> 1 of the samples above and below, or the mean along the best of four diagonals
where x - 3s >= 0 and x + 3s <= C - 1 -- clamped to d +- diff around the temporal mean d = (p2 + n2) >> 1, diff being the largest of
three temporal differences, widened by the spatial-interlacing check where y - 2 >= 0 and y + 2 <= R - 1.  Samples at depth d are read
as min(s, 2^d - 1); kept rows are copied as they are.

How far ffmpeg is followed: the arithmetic of an interior sample is yadif's.  The two border conditions (x +- 3s, y +- 2) and the
mirrored up / dn rows are this project's; ffmpeg's edge handling differs in the outermost rows and columns.  ffmpeg is not available
where this was written, so nothing here is pinned to its output.  Telecined film is not for this module (3:2 pulldown material becomes 60p with
repeated pictures: savsr_amd/pulldown.py, `pulldown=`, recovers the film frames instead), the temporal taps read across scene cuts as yadif's do (there the clamp widens and the spatial prediction stands),
and the default rule is yadif's.  method="bwdif" (`bwdif_matrix`, below) keeps yadif's temporal clamp and interpolates with the w3fdif filters
of ffmpeg's `bwdif` instead; rate="same" returns the first field in time of every source frame only (N frames, the frames [0::2] of the
2N).  Neither is a learned rule.

`savsr_amd.deinterlace` names this module and, called, the GPU function: `savsr_amd.deinterlace(frames, order, ...)` is
`savsr_amd.prepass.deinterlace` (the module object is callable, below: the package's public surface names both, and a function of that
name in the package would shadow this module).  importlib.reload keeps it callable and its functions pickle by reference
(tests/test_deinterlace.py).
"""
from __future__ import annotations

import sys
import types
from typing import Dict, Optional, Tuple

import numpy as np

from .frames import check_pixel_format, layout_of
from .yuv import MONO, check_depth, frame_bytes, layout_name, luma_plane, split_planes

FIELD_ORDERS = ("tff", "bff")
# what `deinterlace_matrix` counts: each of the four CHECKs taken, the diff widened by the interlacing check, the result clamped low / high
BRANCHES = ("check_m1", "check_m2", "check_p1", "check_p2", "widened", "clamp_lo", "clamp_hi")
MAX_STEP = 4
DEINTERLACERS = ("yadif", "bwdif")
FIELD_RATES = ("double", "same")
# what `bwdif_matrix` counts: diff == 0 (the woven sample); among the other samples the three interpolations (the high-frequency filter,
# the spatial one, the two-tap mean of the rows without y +- 4), the clamp widened, the interpolation clamped low / high, the clamped
# value clipped to 0 / 2^depth - 1
BWDIF_BRANCHES = ("still", "line_hf", "line_sp", "edge", "widened", "clamp_lo", "clamp_hi", "clip_lo", "clip_hi")
BWDIF_LF = (4309, 213)
BWDIF_HF = (5570, 3801, 1016)
BWDIF_SP = (5077, 981)


def check_order(order, what: str = "order") -> int:
    """The id of a field order: 0 = "tff" (top field first), 1 = "bff"."""
    if not isinstance(order, str) or order not in FIELD_ORDERS:
        raise ValueError(f"{what} = {order!r}: one of {', '.join(FIELD_ORDERS)}")
    return FIELD_ORDERS.index(order)


def kept_parity(order: str, f: int) -> int:
    """p: output frame 2n + f keeps the rows y with y % 2 == p."""
    return f if check_order(order) == 0 else 1 - f


def check_method(method, what: str = "method") -> int:
    """The id of a deinterlacer: 0 = "yadif", 1 = "bwdif"."""
    if not isinstance(method, str) or method not in DEINTERLACERS:
        raise ValueError(f"{what} = {method!r}: one of {', '.join(DEINTERLACERS)}")
    return DEINTERLACERS.index(method)


def check_rate(rate, what: str = "rate") -> int:
    """The id of a field rate: 0 = "double" (2N frames), 1 = "same" (N frames: the first field in time of every source frame)."""
    if not isinstance(rate, str) or rate not in FIELD_RATES:
        raise ValueError(f"{what} = {rate!r}: one of {', '.join(FIELD_RATES)}")
    return FIELD_RATES.index(rate)


def _cols(a: np.ndarray, k: int) -> np.ndarray:
    """a[..., x + k] for every x (wrapped at the ends: the caller uses it only where x + k lies inside the row)."""
    return np.roll(a, -k, axis=-1)


def deinterlace_matrix(mats, order: str, step: int = 1, depth: int = 8) -> Tuple[np.ndarray, Dict[str, int]]:
    """[N, R, C] integer samples -> ([2N, R, C] of the same dtype, the count of interpolated samples per branch of BRANCHES): the rule of
    the module's docstring on every matrix, with pixel step `step` (1 .. 4, dividing C).  R >= 2 and C >= 1."""
    check_order(order)
    m = np.asarray(mats)
    if m.ndim != 3 or m.dtype.kind not in "iu":
        raise ValueError(f"matrices must be [N, R, C] integers, got {m.dtype} {tuple(m.shape)}")
    N, R, C = m.shape
    if N < 1:
        raise ValueError("the video has no frames")
    if R == 1:
        raise ValueError("R = 1: a matrix of one row has no second field to interpolate from (R >= 2)")
    if R < 2 or C < 1:
        raise ValueError(f"a matrix of {R} x {C}: R >= 2 and C >= 1")
    if isinstance(step, bool) or not isinstance(step, (int, np.integer)) or not 1 <= step <= MAX_STEP or C % step:
        raise ValueError(f"step = {step!r}: 1 .. {MAX_STEP} and a divisor of C = {C}")
    if depth not in (8, 10, 12):
        raise ValueError(f"depth = {depth!r}: 8, 10 or 12")
    s = int(step)
    v = np.minimum(m.astype(np.int64), (1 << depth) - 1)
    out = np.repeat(m, 2, axis=0)          # kept rows: copied as they are
    counts = dict.fromkeys(BRANCHES, 0)
    x = np.arange(C)
    edge = (x - 3 * s >= 0) & (x + 3 * s <= C - 1)
    for n in range(N):
        cur, prev, nxt = v[n], v[max(n - 1, 0)], v[min(n + 1, N - 1)]
        for f in (0, 1):
            p = kept_parity(order, f)
            p2, n2 = (prev, cur) if f == 0 else (cur, nxt)
            ys = np.arange(1 - p, R, 2)
            if ys.size == 0:
                continue
            up = np.where(ys == 0, ys + 1, ys - 1)
            dn = np.where(ys == R - 1, ys - 1, ys + 1)
            U, D = cur[up], cur[dn]
            c, e = U, D
            d = (p2[ys] + n2[ys]) >> 1
            t0 = np.abs(p2[ys] - n2[ys])
            t1 = (np.abs(prev[up] - c) + np.abs(prev[dn] - e)) >> 1
            t2 = (np.abs(nxt[up] - c) + np.abs(nxt[dn] - e)) >> 1
            diff = np.maximum(np.maximum(t0 >> 1, t1), t2)
            pred = (c + e) >> 1
            score = np.abs(_cols(U, -s) - _cols(D, -s)) + np.abs(c - e) + np.abs(_cols(U, s) - _cols(D, s)) - 1

            def check(j, allowed, score, pred):
                sc = (np.abs(_cols(U, (j - 1) * s) - _cols(D, -(j + 1) * s)) + np.abs(_cols(U, j * s) - _cols(D, -j * s))
                      + np.abs(_cols(U, (j + 1) * s) - _cols(D, -(j - 1) * s)))
                taken = allowed & (sc < score)
                return taken, np.where(taken, sc, score), np.where(taken, (_cols(U, j * s) + _cols(D, -j * s)) >> 1, pred)

            all_edge = np.broadcast_to(edge, U.shape)
            m1, score, pred = check(-1, all_edge, score, pred)
            m2, score, pred = check(-2, m1, score, pred)
            p1, score, pred = check(1, all_edge, score, pred)
            q2, score, pred = check(2, p1, score, pred)
            inner = ((ys - 2 >= 0) & (ys + 2 <= R - 1))[:, None]
            ym, yp = np.clip(ys - 2, 0, R - 1), np.clip(ys + 2, 0, R - 1)
            b = (p2[ym] + n2[ym]) >> 1
            g = (p2[yp] + n2[yp]) >> 1
            mx = np.maximum(np.maximum(d - e, d - c), np.minimum(b - c, g - e))
            mn = np.minimum(np.minimum(d - e, d - c), np.maximum(b - c, g - e))
            wide = np.where(inner, np.maximum(np.maximum(diff, mn), -mx), diff)
            res = np.minimum(np.maximum(pred, d - wide), d + wide)
            out[2 * n + f, ys] = res.astype(m.dtype)
            for name, mask in zip(BRANCHES, (m1, m2, p1, q2, wide > diff, pred < d - wide, pred > d + wide)):
                counts[name] += int(np.count_nonzero(mask))
    return out, counts


def bwdif_matrix(mats, order: str, depth: int = 8) -> Tuple[np.ndarray, Dict[str, int]]:
    """[N, R, C] integer samples -> ([2N, R, C] of the same dtype, the count of interpolated samples per branch of BWDIF_BRANCHES): the
    rule of ffmpeg's `bwdif` filter (yadif's temporal clamp around the w3fdif interpolation filters) with the conventions of
    `deinterlace_matrix`: the kept rows, cur / prev / next, p2 / n2, up / dn and min(s, 2^depth - 1) are the module docstring's.  There
    are no horizontal taps, so there is no pixel step: packed frames are their h x (w * c) byte matrix, sample by sample.  R >= 2, C >= 1.

    For an interpolated sample (y, x), with c = cur[up], e = cur[dn], d = (p2[y] + n2[y]) >> 1:
      t0 = |p2[y] - n2[y]|, t1 = (|prev[up] - c| + |prev[dn] - e|) >> 1, t2 the same with next, diff = max(t0 >> 1, t1, t2)  (yadif's)
      inner (y - 2 >= 0 and y + 2 <= R - 1): b = ((p2[y-2] + n2[y-2]) >> 1) - c, g = ((p2[y+2] + n2[y+2]) >> 1) - e,
        mx = max(d - e, d - c, min(b, g)), mn = min(d - e, d - c, max(b, g)), wide = max(diff, mn, -mx); elsewhere wide = diff
      line (y - 4 >= 0 and y + 4 <= R - 1) and |c - e| > t0:
        interp = (((HF0 (p2[y] + n2[y]) - HF1 (p2[y-2] + n2[y-2] + p2[y+2] + n2[y+2]) + HF2 (p2[y-4] + n2[y-4] + p2[y+4] + n2[y+4])) >> 2)
                  + LF0 (c + e) - LF1 (cur[y-3] + cur[y+3])) >> 13
      line and |c - e| <= t0: interp = (SP0 (c + e) - SP1 (cur[y-3] + cur[y+3])) >> 13
      not line: interp = (c + e) >> 1
      result: d where diff == 0 (so static video comes back as it is), else clip(min(max(interp, d - wide), d + wide), 0, 2^depth - 1)
    Every >> is an arithmetic shift: the floor of the division, also of a negative value (numpy's and Python's >>; the kernels shift
    signed 32-bit integers, which does the same).  Every intermediate fits 32 bits at 12 bits (the largest is below 6.3e7).  The
    counts other than "still" are taken among the samples with diff != 0, the ones whose result they decide.

    How far ffmpeg is followed: the arithmetic of an interior sample is bwdif's (vf_bwdif.c's constants and order of operations).  The
    `inner` and `line` border conditions, the mirrored up / dn rows and the clamped first and last frame are this project's; ffmpeg
    filters the first and the last field with an intra-only filter, which is not modelled.  ffmpeg is not available where this was
    written, so nothing here is pinned to its output."""
    check_order(order)
    m = np.asarray(mats)
    if m.ndim != 3 or m.dtype.kind not in "iu":
        raise ValueError(f"matrices must be [N, R, C] integers, got {m.dtype} {tuple(m.shape)}")
    N, R, C = m.shape
    if N < 1:
        raise ValueError("the video has no frames")
    if R == 1:
        raise ValueError("R = 1: a matrix of one row has no second field to interpolate from (R >= 2)")
    if R < 2 or C < 1:
        raise ValueError(f"a matrix of {R} x {C}: R >= 2 and C >= 1")
    if depth not in (8, 10, 12):
        raise ValueError(f"depth = {depth!r}: 8, 10 or 12")
    top = (1 << depth) - 1
    v = np.minimum(m.astype(np.int64), top)
    out = np.repeat(m, 2, axis=0)          # kept rows: copied as they are
    counts = dict.fromkeys(BWDIF_BRANCHES, 0)
    (LF0, LF1), (HF0, HF1, HF2), (SP0, SP1) = BWDIF_LF, BWDIF_HF, BWDIF_SP
    for n in range(N):
        cur, prev, nxt = v[n], v[max(n - 1, 0)], v[min(n + 1, N - 1)]
        for f in (0, 1):
            p = kept_parity(order, f)
            p2, n2 = (prev, cur) if f == 0 else (cur, nxt)
            ys = np.arange(1 - p, R, 2)
            if ys.size == 0:
                continue
            up = np.where(ys == 0, ys + 1, ys - 1)
            dn = np.where(ys == R - 1, ys - 1, ys + 1)

            def row(k):          # (clipped: read only where `inner` / `line` says the row exists)
                return np.clip(ys + k, 0, R - 1)

            c, e = cur[up], cur[dn]
            s0 = p2[ys] + n2[ys]
            d = s0 >> 1
            t0 = np.abs(p2[ys] - n2[ys])
            t1 = (np.abs(prev[up] - c) + np.abs(prev[dn] - e)) >> 1
            t2 = (np.abs(nxt[up] - c) + np.abs(nxt[dn] - e)) >> 1
            diff = np.maximum(np.maximum(t0 >> 1, t1), t2)
            inner = np.broadcast_to(((ys - 2 >= 0) & (ys + 2 <= R - 1))[:, None], c.shape)
            line = np.broadcast_to(((ys - 4 >= 0) & (ys + 4 <= R - 1))[:, None], c.shape)
            sm, sp = p2[row(-2)] + n2[row(-2)], p2[row(2)] + n2[row(2)]
            b, g = (sm >> 1) - c, (sp >> 1) - e
            mx = np.maximum(np.maximum(d - e, d - c), np.minimum(b, g))
            mn = np.minimum(np.minimum(d - e, d - c), np.maximum(b, g))
            wide = np.where(inner, np.maximum(np.maximum(diff, mn), -mx), diff)
            far = p2[row(-4)] + n2[row(-4)] + p2[row(4)] + n2[row(4)]
            c3 = cur[row(-3)] + cur[row(3)]
            hf = (((HF0 * s0 - HF1 * (sm + sp) + HF2 * far) >> 2) + LF0 * (c + e) - LF1 * c3) >> 13
            spat = (SP0 * (c + e) - SP1 * c3) >> 13
            use_hf = np.abs(c - e) > t0
            interp = np.where(line, np.where(use_hf, hf, spat), (c + e) >> 1)
            clamped = np.minimum(np.maximum(interp, d - wide), d + wide)
            still = diff == 0
            res = np.where(still, d, np.clip(clamped, 0, top))
            out[2 * n + f, ys] = res.astype(m.dtype)
            moving = ~still
            for name, mask in zip(BWDIF_BRANCHES, (still, moving & line & use_hf, moving & line & ~use_hf, moving & ~line, moving & (wide > diff),
                                                   moving & (interp < d - wide), moving & (interp > d + wide), moving & (clamped < 0),
                                                   moving & (clamped > top))):
                counts[name] += int(np.count_nonzero(mask))
    return out, counts


def _planes(frames: np.ndarray, h: int, w: int, depth: int, layout: str):
    if layout == MONO:
        return [luma_plane(frames, h, w, depth, MONO)]
    return list(split_planes(frames, h, w, depth, layout))


def check_frame_rows(h: int, layout: Optional[str]) -> None:
    """Every matrix of a frame has two rows: h >= 2, and h >= 3 for 4:2:0, whose chroma planes have (h + 1) // 2."""
    if h == 1:
        raise ValueError("frames of one row (R = 1) have no second field to interpolate from: h >= 2")
    if layout == "420" and h < 3:
        raise ValueError(f"4:2:0 frames of {h} rows have chroma planes of one row (R = 1): interlaced 4:2:0 needs h >= 3")


def deinterlace_frames_counted(frames, order: str, pixel_format: str = "rgb", size=None, depth: int = 8, method: str = "yadif",
                               rate: str = "double") -> Tuple[np.ndarray, Dict[str, int]]:
    """`deinterlace_frames` and the branch counts summed over the matrices (BRANCHES for "yadif", BWDIF_BRANCHES for "bwdif"; of both
    fields of every frame, also with rate="same")."""
    check_order(order)
    bwdif, same = check_method(method) == 1, check_rate(rate) == 1
    names = BWDIF_BRANCHES if bwdif else BRANCHES
    hw = check_pixel_format(pixel_format, size)
    if hasattr(frames, "detach"):
        frames = frames.detach().cpu().numpy()
    frames = np.asarray(frames)
    counts = dict.fromkeys(names, 0)

    def run(mats, step, d):
        res, cnt = bwdif_matrix(mats, order, d) if bwdif else deinterlace_matrix(mats, order, step, d)
        for k in names:
            counts[k] += cnt[k]
        return res[0::2] if same else res          # rate "same": the first field in time of every source frame

    if hw:
        h, w = hw
        layout, depth = layout_of(pixel_format), check_depth(depth)
        fb = frame_bytes(h, w, depth, layout)
        if frames.dtype != np.uint8 or frames.ndim != 2 or frames.shape[1] != fb:
            raise ValueError(f"{'' if depth == 8 else f'{depth}-bit '}{layout_name(layout)} frames of {h} x {w} are [N, {fb}] uint8, "
                             f"got {frames.dtype} {tuple(frames.shape)}")
        check_frame_rows(h, layout)
        planes = [run(p, 1, depth) for p in _planes(frames, h, w, depth, layout)]
        n2 = planes[0].shape[0]
        return np.concatenate([np.ascontiguousarray(p.astype(np.uint8 if depth == 8 else "<u2")).reshape(n2, -1).view(np.uint8) for p in planes], 1), counts
    if depth != 8:
        raise ValueError(f"depth = {depth} goes with pixel_format = 'i420', 'i422', 'i444' or 'y400': packed frames are 8-bit")
    if frames.dtype.kind == "f":
        raise ValueError("float frames have no integer samples to deinterlace: give [N, h, w, c] uint8 or planar frames (quantise first)")
    if frames.dtype != np.uint8 or frames.ndim != 4:
        raise ValueError(f"frames must be [N, h, w, c] uint8, got {frames.dtype} {tuple(frames.shape)}")
    n, h, w, c = frames.shape
    if not 1 <= c <= MAX_STEP:
        raise ValueError(f"frames have {c} channels: 1 .. {MAX_STEP}")
    check_frame_rows(h, None)
    return run(frames.reshape(n, h, w * c), c, 8).reshape(-1, h, w, c), counts


def deinterlace_frames(frames, order: str, pixel_format: str = "rgb", size=None, depth: int = 8, method: str = "yadif",
                       rate: str = "double") -> np.ndarray:
    """2N progressive frames of N interlaced ones, in the same format (method: one of DEINTERLACERS, `deinterlace_matrix` or
    `bwdif_matrix` on every matrix; rate "same": N frames, the frames [0::2] of the 2N, the first field in time of every source frame).  [N, h, w, c] uint8: the h x (w * c) byte matrix with step c.
    Planar frames (pixel_format "i420", "i422", "i444", "y400" with size=(h, w); [N, frame_bytes] uint8, little-endian 16-bit words at
    depth 10 / 12): every plane with step 1, the chroma planes with the parity of the luma plane (in interlaced 4:2:0 the chroma rows
    alternate between the fields as the luma rows do).  Float frames are refused."""
    return deinterlace_frames_counted(frames, order, pixel_format, size, depth, method, rate)[0]


# ---- the command line's header decision -----------------------------------------------------------------------------------------------------
FIELD_FLAGS = ("progressive", "auto") + FIELD_ORDERS


def resolve_fields(flag: Optional[str], tag: Optional[str], fps: Tuple[int, int], rate: str = "double"):
    """--fields and the input's interlace tag -> (order or None, the output's interlace tag, the output's frame rate, a note for stderr
    or None).  flag: one of FIELD_FLAGS, or None when --fields was not given; tag: the Y4M input's I tag ("p", "t", "b", "m"; "?" reads
    as progressive), None for a PNG folder.  Without fields the tag and the rate pass through; with fields the output is progressive at
    twice the rate (rate="same": at the input's rate).  auto: It -> tff, Ib -> bff, Ip -> progressive; Im (mixed) and a PNG folder are refused."""
    if flag is not None and flag not in FIELD_FLAGS:
        raise ValueError(f"--fields = {flag!r}: one of {', '.join(FIELD_FLAGS)}")
    same = check_rate(rate, "--field-rate") == 1
    keep = "p" if tag is None else tag
    if flag is None or flag == "progressive":
        note = None
        if flag is None and tag in ("t", "b", "m"):
            note = (f"the input is tagged interlaced (I{tag}) and is being treated as progressive: woven fields go through the network as they "
                    f"are; give --fields auto (or tff / bff) to deinterlace first")
        return None, keep, (int(fps[0]), int(fps[1])), note
    if flag == "auto":
        if tag is None:
            raise ValueError("--fields auto reads the Y4M input's I tag; a PNG folder has none: give --fields tff or --fields bff")
        if tag == "m":
            raise ValueError("--fields auto: the input is tagged Im (mixed progressive and interlaced frames), which is not modelled; give "
                             "--fields tff or --fields bff to treat every frame as interlaced")
        if tag not in ("t", "b"):
            return None, keep, (int(fps[0]), int(fps[1])), None
        order = "tff" if tag == "t" else "bff"
    else:
        order = flag
    return order, "p", ((1 if same else 2) * int(fps[0]), int(fps[1])), None


class _CallableModule(types.ModuleType):
    """savsr_amd.deinterlace(frames, order, pixel_format="rgb", size=None, depth=8, method="yadif", rate="double"): 2N (rate "same":
    N) progressive frames on the GPU (savsr_amd.prepass.deinterlace, which `deinterlace_frames` above specifies bit for bit)."""

    def __call__(self, frames, order, pixel_format: str = "rgb", size=None, depth: int = 8, method: str = "yadif", rate: str = "double"):
        from .prepass import deinterlace
        return deinterlace(frames, order, pixel_format, size, depth, method, rate)


sys.modules[__name__].__class__ = _CallableModule
