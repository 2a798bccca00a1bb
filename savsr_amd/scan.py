"""Scan detection: is a video progressive, interlaced or telecined film, and with which field order -- the host-side specification
(numpy, integers only, no GPU needed).  `fields=` and `pulldown=` rest on the caller knowing the answer; this module finds it from the
content.  The kernels of csrc/scan.hip equal `field_stats` bit for bit; the decision is host work in exact arithmetic.

A frame is a matrix M of R rows x C samples, the project's usual reading: the h x (w * c) bytes of packed uint8 frames, the Y plane of
planar ones; at depth 10 / 12 every sample is read as min(s, 2^d - 1) >> (d - 8), as `pair_sad` and `field_scores` read it.

The comb measure is pulldown.field_scores': comb(a, b, c) = |a - b| + |c - b| - |a - c|, twice the distance of b from the interval its
vertical neighbours a, c span.

`field_stats`: per frame n eight exact integer sums.  With prev = frame max(n - 1, 0), next = frame min(n + 1, N - 1), and for the rows y
of parity q with 1 <= y <= R - 2, a = M[n][y - 1], c = M[n][y + 1]:

    columns 0, 1   comb_prev[q] = sum comb(a, M[prev][y], c)       field q of the previous frame between this frame's other field
    columns 2, 3   comb_next[q] = sum comb(a, M[next][y], c)       field q of the next frame there
    columns 4, 5   comb_self[q] = sum comb(a, M[n][y], c)          the frame's own field q there
    columns 6, 7   rep[q]       = sum |M[n][y] - M[prev][y]| over ALL rows y of parity q: the SAD of field q against the previous frame's

comb_prev[1 - p] and comb_self[1 - p] are pulldown.field_scores(..., order)[:, 0] and [:, 1], p the order's first parity.

`verdict_from_stats`, in this order:

  1. Repeats.  For n >= 1, rep_field[n] = q iff repeat_threshold * rep[n][q] < rep[n][1 - q] (strict: a frame that equals its
     predecessor repeats nothing), else None; rep_field[0] is None.
  2. Telecine.  hits[p] = #{n : 1 <= n <= N - 3, rep_field[n] = p and rep_field[n + 2] = 1 - p}: in AA BB BC CD DD the first field
     repeats in the third frame and the second in the fifth.  Telecine with first parity p iff hits[p] > hits[1 - p], hits[p] >= 2 and
     10 * hits[p] >= N - 3 (the cadence shows in at least half of the cycles).
  3. Totals over the frames 1 .. N - 2, whose neighbours are both real: S = sum comb_self[0] + comb_self[1]; A_tff = sum comb_prev[0] +
     comb_next[1] (the field pairs that lie 1 1/2 frame periods apart if the video is tff); A_bff = sum comb_prev[1] + comb_next[0].
  4. Progressive iff min(A_tff, A_bff) > progressive_threshold * S: a frame's two fields fit each other much better than they fit the
     neighbouring frames'.
  5. Interlaced tff iff A_tff > interlace_threshold * A_bff; bff iff A_bff > interlace_threshold * A_tff.
  6. Undetermined: everything else, and N < 3.  Static, flat or motionless video carries no evidence.

ffmpeg's `idet` is the idea, not the definition: the measure, the rule and the thresholds (5/4, 3/2, 3) are this project's own.  They
separate synthetic moving pictures (sums of sinusoids, with and without noise) and are NOT validated on real footage.  Limits: one verdict
per video, so mixed content is not handled; nor are 2:2 phase-shifted PAL film, cadences other than 3:2, or fades.  Uncorrelated
noise carries no temporal order: the interlace rule may answer anything on it.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction
from typing import Dict, List, Optional, Tuple

import numpy as np

from .deinterlace import FIELD_ORDERS
from .pulldown import _as_numpy, _frame_kind, _planes
from .yuv import check_depth

SCANS = ("progressive", "interlaced", "telecine", "undetermined")
SCAN_FLAGS = ("detect",)
DEFAULT_INTERLACE, DEFAULT_PROGRESSIVE, DEFAULT_REPEAT = Fraction(5, 4), Fraction(3, 2), Fraction(3)
STAT_COLUMNS = 8


def check_scan_threshold(value, what: str) -> Fraction:
    """A threshold as an exact fraction; refuses a non-number, a non-finite and a non-positive one (as scenes.check_threshold does)."""
    if isinstance(value, bool) or not isinstance(value, (int, float, Fraction, np.integer)):
        raise ValueError(f"{what} must be a positive number, got {value!r}")
    if isinstance(value, float) and not math.isfinite(value):
        raise ValueError(f"{what} must be finite, got {value!r}")
    thr = Fraction(int(value) if isinstance(value, np.integer) else value)
    if thr <= 0:
        raise ValueError(f"{what} must be positive, got {value!r}")
    return thr


def check_thresholds(interlace_threshold, progressive_threshold, repeat_threshold) -> Tuple[Fraction, Fraction, Fraction]:
    return (check_scan_threshold(interlace_threshold, "interlace_threshold"), check_scan_threshold(progressive_threshold, "progressive_threshold"),
            check_scan_threshold(repeat_threshold, "repeat_threshold"))


def check_scan(scan) -> Optional[str]:
    """scan is None or "detect"."""
    if scan is None:
        return None
    if not isinstance(scan, str) or scan not in SCAN_FLAGS:
        raise ValueError(f"scan = {scan!r}: None or 'detect' (find out from the content whether the video is progressive, interlaced or "
                         f"telecined film; an explicit answer is fields= or pulldown=)")
    return scan


def comb(a, b, c):
    """|a - b| + |c - b| - |a - c| on integer arrays: never negative."""
    return np.abs(a - b) + np.abs(c - b) - np.abs(a - c)


def field_stats(mats, depth: int = 8) -> np.ndarray:
    """[N, R, C] integer samples -> [N, 8] int64: the sums of the module's docstring.  R < 3 gives zero comb sums; rep is defined from
    R >= 1."""
    m = np.asarray(mats)
    if m.ndim != 3 or m.dtype.kind not in "iu":
        raise ValueError(f"matrices must be [N, R, C] integers, got {m.dtype} {tuple(m.shape)}")
    depth = check_depth(depth)
    v = np.minimum(m.astype(np.int64), (1 << depth) - 1) >> (depth - 8)
    N, R, _ = v.shape
    out = np.zeros((N, STAT_COLUMNS), dtype=np.int64)
    for n in range(N):
        prev, nxt = v[max(n - 1, 0)], v[min(n + 1, N - 1)]
        for q in (0, 1):
            ys = np.arange(q, R, 2)
            out[n, 6 + q] = np.abs(v[n][ys] - prev[ys]).sum(dtype=np.int64)
            ys = ys[(ys >= 1) & (ys <= R - 2)]
            if ys.size:
                a, c = v[n][ys - 1], v[n][ys + 1]
                for col, src in ((0, prev), (2, nxt), (4, v[n])):
                    out[n, col + q] = comb(a, src[ys], c).sum(dtype=np.int64)
    return out


def frame_stats(frames, pixel_format: str = "rgb", size=None, depth: int = 8) -> np.ndarray:
    """`field_stats` of frames: every byte of packed [N, h, w, c] uint8 frames, the Y plane of planar ones (pulldown.frame_scores'
    frames and refusals)."""
    frames = _as_numpy(frames)
    hw, layout, depth = _frame_kind(frames, pixel_format, size, depth)
    return field_stats(_planes(frames, hw, layout, depth)[0], depth)


@dataclass(frozen=True)
class ScanVerdict:
    """What `verdict_from_stats` found.  scan: one of SCANS; order: "tff" / "bff" for interlaced and telecine, else None; s, a_tff, a_bff:
    the totals of step 3; hits: (hits[0], hits[1]); rep_field: per frame 0, 1 or None; the thresholds as exact fractions."""
    scan: str
    order: Optional[str]
    s: int
    a_tff: int
    a_bff: int
    hits: Tuple[int, int]
    rep_field: Tuple[Optional[int], ...]
    interlace_threshold: Fraction = DEFAULT_INTERLACE
    progressive_threshold: Fraction = DEFAULT_PROGRESSIVE
    repeat_threshold: Fraction = DEFAULT_REPEAT

    def kwargs(self) -> Dict[str, str]:
        """The explicit arguments of upscale_video / VideoUpscaler that say what was found: {"fields": order}, {"pulldown": order} or {}
        (progressive; undetermined reads as progressive: the path as it was)."""
        if self.scan == "interlaced":
            return {"fields": self.order}
        if self.scan == "telecine":
            return {"pulldown": self.order}
        return {}

    def flag(self) -> Optional[str]:
        """The command line's equivalent: "--fields tff", "--pulldown bff", ... or None."""
        return {"interlaced": f"--fields {self.order}", "telecine": f"--pulldown {self.order}"}.get(self.scan)

    def describe(self) -> str:
        name = {"tff": "top field first", "bff": "bottom field first"}.get(self.order)
        return self.scan if name is None else f"{self.scan}, {name}"

    def as_json(self) -> dict:
        """What --scan-out writes."""
        return {"scan": self.scan, "order": self.order, "totals": {"S": self.s, "A_tff": self.a_tff, "A_bff": self.a_bff},
                "hits": list(self.hits), "rep_field": list(self.rep_field),
                "thresholds": {"interlace": str(self.interlace_threshold), "progressive": str(self.progressive_threshold),
                               "repeat": str(self.repeat_threshold)}}


def verdict_from_stats(stats, interlace_threshold=DEFAULT_INTERLACE, progressive_threshold=DEFAULT_PROGRESSIVE,
                       repeat_threshold=DEFAULT_REPEAT) -> ScanVerdict:
    """The decision of the module's docstring on `field_stats`' rows, in exact integer / Fraction arithmetic."""
    ti, tp, tr = check_thresholds(interlace_threshold, progressive_threshold, repeat_threshold)
    st = np.asarray(stats)
    if st.ndim != 2 or st.shape[1] != STAT_COLUMNS or st.dtype.kind not in "iu":
        raise ValueError(f"stats must be [N, {STAT_COLUMNS}] integers, got {st.dtype} {tuple(st.shape)}")
    rows: List[List[int]] = [[int(v) for v in r] for r in st.tolist()]
    N = len(rows)
    rep_field: List[Optional[int]] = [None] * N
    for n in range(1, N):
        rep = rows[n][6:8]
        for q in (0, 1):
            if tr * rep[q] < rep[1 - q]:
                rep_field[n] = q
    hits = [0, 0]
    for n in range(1, N - 2):
        p = rep_field[n]
        if p is not None and rep_field[n + 2] == 1 - p:
            hits[p] += 1
    inner = rows[1:N - 1] if N >= 3 else []
    S = sum(r[4] + r[5] for r in inner)
    A_tff = sum(r[0] + r[3] for r in inner)
    A_bff = sum(r[1] + r[2] for r in inner)

    def verdict(scan, order=None):
        return ScanVerdict(scan, order, S, A_tff, A_bff, (hits[0], hits[1]), tuple(rep_field), ti, tp, tr)

    if N < 3:
        return verdict("undetermined")
    for p in (0, 1):
        if hits[p] > hits[1 - p] and hits[p] >= 2 and 10 * hits[p] >= N - 3:
            return verdict("telecine", FIELD_ORDERS[p])
    if min(A_tff, A_bff) > tp * S:
        return verdict("progressive")
    if A_tff > ti * A_bff:
        return verdict("interlaced", "tff")
    if A_bff > ti * A_tff:
        return verdict("interlaced", "bff")
    return verdict("undetermined")


def detect_scan_frames(frames, pixel_format: str = "rgb", size=None, depth: int = 8, interlace_threshold=DEFAULT_INTERLACE,
                       progressive_threshold=DEFAULT_PROGRESSIVE, repeat_threshold=DEFAULT_REPEAT) -> ScanVerdict:
    """verdict_from_stats(frame_stats(...)): what savsr_amd.detect_scan computes, on the host."""
    check_thresholds(interlace_threshold, progressive_threshold, repeat_threshold)
    return verdict_from_stats(frame_stats(frames, pixel_format, size, depth), interlace_threshold, progressive_threshold, repeat_threshold)


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
def tag_note(verdict: ScanVerdict, tag: Optional[str]) -> Optional[str]:
    """The stderr line for a Y4M input whose I tag says something else than the content; None when they agree, when there is no tag (a PNG
    folder) and when nothing was determined."""
    if tag is None or verdict.scan == "undetermined":
        return None
    if tag == {"tff": "t", "bff": "b"}.get(verdict.order, "p"):          # (telecined film lies in interlaced frames: It / Ib agree with it)
        return None
    return f"--scan detect: the input is tagged I{tag}, its content is {verdict.describe()}: the content is followed"
