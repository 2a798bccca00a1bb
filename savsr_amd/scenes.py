"""Scene cuts in the sequence path: the host-side specification (numpy / pure Python, no GPU needed).

A cut list is a strictly increasing list of frame indices k, 0 < k < N; frame k is the first frame of a new scene.  The cuts split
[0, N) into segments [a, b), and a segment is treated as the reference treats a folder: output frame i of segment [a, b) has the window
a + window_indices(i - a, b - a, num_frame, mode), mode = the call's padding if check_length(b - a, num_frame, padding) passes and
"replicate" otherwise (`scene_windows`).  upscale_video(v, cuts=...) is therefore, bit for bit, the concatenation of upscale_video on
the segments.

The detector: per pair of consecutive frames the sum of absolute differences of their 8-bit samples (`pair_sad`, the specification of
savsr_video_pair_sad_u8 / _i420 / _i420_16 / _yuvp / _f32 in csrc/scene.hip), then ffmpeg scdet's rule in exact arithmetic (`cuts_from_sad`).

`ScenePlan` is the streaming form's bookkeeping (VideoUpscaler with cuts): which frames can be returned, with which windows, and which
past frames must be kept, when cuts and the end of the video are only known up to the last pushed frame.
"""
from __future__ import annotations

import math
from bisect import bisect_right
from fractions import Fraction
from functools import lru_cache
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .harness import window_indices
from .frames import check_length, check_padding, check_pixel_format, chroma_of
from .yuv import LUMA_FORMAT, MONO, check_depth, frame_bytes, layout_name, luma_plane, split_planes


# ---- the detector --------------------------------------------------------------------------------------------------------------------
def quantize_u8(x: np.ndarray) -> np.ndarray:
    """savsr_video_quantize_u8's value of every float: clamp to [0, 1] (fmaxf / fminf: NaN -> 0), x 255.0f, round half to even."""
    x = np.asarray(x, dtype=np.float32)
    return np.rint(np.fmin(np.fmax(x, np.float32(0)), np.float32(1)) * np.float32(255)).astype(np.uint8)


def _samples_of(frames, pixel_format: str, size, depth: int = 8) -> np.ndarray:
    """[N, S] uint8: the samples the detector compares, frame by frame."""
    i420 = check_pixel_format(pixel_format, size)
    if hasattr(frames, "detach"):
        frames = frames.detach().cpu().numpy()
    frames = np.asarray(frames)
    if i420 and pixel_format == LUMA_FORMAT:          # grey-scale frames: the Y plane is the frame
        y = luma_plane(frames, i420[0], i420[1], check_depth(depth), MONO)
        return (np.minimum(y, (1 << depth) - 1) >> (depth - 8)).astype(np.uint8).reshape(y.shape[0], -1)
    if depth != 8:
        depth = check_depth(depth)
        if not i420:
            raise ValueError(f"depth = {depth} goes with pixel_format = 'i420', 'i422' or 'i444': it is the bit depth of YUV input")
        y = split_planes(frames, i420[0], i420[1], depth, chroma_of(pixel_format))[0]
        return (np.minimum(y, np.uint16((1 << depth) - 1)) >> (depth - 8)).astype(np.uint8).reshape(y.shape[0], -1)
    if i420:
        h, w = i420
        chroma = chroma_of(pixel_format)
        if frames.dtype != np.uint8 or frames.ndim != 2 or frames.shape[1] != frame_bytes(h, w, 8, chroma):
            raise ValueError(f"{layout_name(chroma)} frames of {h} x {w} are [N, {frame_bytes(h, w, 8, chroma)}] uint8, "
                             f"got {frames.dtype} {tuple(frames.shape)}")
        return frames[:, :h * w]
    if frames.ndim != 4:
        raise ValueError(f"frames must be [N, h, w, c] uint8 or [N, c, h, w] float, got {frames.ndim} dimensions")
    if frames.dtype == np.uint8:
        return frames.reshape(frames.shape[0], -1)
    if frames.dtype.kind != "f":
        raise ValueError(f"frames must be uint8 or float, got {frames.dtype}")
    return quantize_u8(frames).reshape(frames.shape[0], -1)


def sad_samples(shape: Sequence[int], pixel_format: str = "rgb", size=None) -> int:
    """S, the samples compared per pair: c * h * w of RGB frames (either layout), h * w (the Y plane) of YUV frames (i420, i422, i444)."""
    i420 = check_pixel_format(pixel_format, size)
    if i420:
        return i420[0] * i420[1]
    if len(shape) != 4:
        raise ValueError(f"frames must be [N, h, w, c] uint8 or [N, c, h, w] float, got {len(shape)} dimensions")
    return int(shape[1]) * int(shape[2]) * int(shape[3])


def pair_sad(frames, pixel_format: str = "rgb", size=None, depth: int = 8) -> np.ndarray:
    """int64 [N - 1]: entry j is the sum of absolute differences of the 8-bit samples of frames j and j + 1.
    [N, h, w, c] uint8: every byte.  I420 ([N, i420_bytes(h, w)] uint8, size=(h, w)): the Y plane only.  [N, c, h, w] float: every value
    after `quantize_u8`.  depth = 10, 12 (I420 frames of 16-bit samples, [N, 2 * i420_bytes(h, w)] uint8): the Y plane's samples as their 8
    most significant bits, min(s, 2^depth - 1) >> (depth - 8), so the scores -- and with them the threshold -- keep the 8-bit scale.
    pixel_format = "i422" / "i444": the Y plane of those layouts (the first h * w samples of a frame), exactly as for I420."""
    s = _samples_of(frames, pixel_format, size, depth).astype(np.int64)
    if s.shape[0] < 1:
        raise ValueError("the video has no frames")
    return np.abs(s[1:] - s[:-1]).sum(axis=1, dtype=np.int64)


def check_threshold(threshold) -> Fraction:
    """The threshold as an exact fraction; refuses a non-number, a non-finite and a non-positive one."""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, Fraction)):
        raise ValueError(f"scene_threshold must be a positive number (per cent of the largest possible change), got {threshold!r}")
    if isinstance(threshold, float) and not math.isfinite(threshold):
        raise ValueError(f"scene_threshold must be finite, got {threshold!r}")
    thr = Fraction(threshold)
    if thr <= 0:
        raise ValueError(f"scene_threshold must be positive, got {threshold!r}")
    return thr


def cuts_from_sad(sad: Sequence[int], samples: int, threshold=10.0, first: int = 1, prev: int = 0) -> List[int]:
    """The cuts among frames first .. first + len(sad) - 1, from sad[j] = the score of the pair (first + j - 1, first + j).
    ffmpeg scdet's rule in exact arithmetic: with s the pair's score and p the previous pair's (`prev` for the first entry; 0 for
    the pair that does not exist before frame 1), m = min(s, |s - p|), and the frame is a cut iff m * 100 >= threshold * 255 * samples.
    Causal: the decision on frame k needs frames k - 2 .. k, which is what lets VideoUpscaler carry `prev` from push to push."""
    thr = check_threshold(threshold)
    if samples < 1:
        raise ValueError(f"samples = {samples}: a pair compares at least one sample")
    bound = thr * 255 * int(samples)
    cuts, p = [], int(prev)
    for j, s in enumerate(sad):
        s = int(s)
        if min(s, abs(s - p)) * 100 >= bound:
            cuts.append(first + j)
        p = s
    return cuts


# ---- segments and their windows ----------------------------------------------------------------------------------------------------------
def check_cuts(cuts, n: Optional[int]) -> List[int]:
    """The cut list as ints: strictly increasing, 0 < k < n (n = None: the length is not known yet, only 0 < k is checked)."""
    if isinstance(cuts, (str, bytes)) or not hasattr(cuts, "__iter__"):
        raise ValueError(f"cuts must be None, 'auto' or a sequence of frame indices, got {cuts!r}")
    out: List[int] = []
    for k in cuts:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"cuts must be frame indices (ints), got {k!r}")
        k = int(k)
        if k <= 0 or (n is not None and k >= n):
            raise ValueError(f"cut {k}: a cut is the first frame of a new scene, 0 < k < {'N' if n is None else n}")
        if out and k <= out[-1]:
            raise ValueError(f"cuts must be strictly increasing, got {k} after {out[-1]}")
        out.append(k)
    return out


def segments(n: int, cuts: Sequence[int]) -> List[Tuple[int, int]]:
    """The segments [a, b) the cuts split [0, n) into."""
    edges = [0] + list(cuts) + [n]
    return list(zip(edges[:-1], edges[1:]))


@lru_cache(maxsize=None)
def min_length(num_frame: int, padding: str) -> int:
    """The shortest video check_length accepts with this padding (every longer one passes as well: the windows reach a fixed number
    of frames past either end)."""
    n = 1
    while True:
        try:
            check_length(n, num_frame, padding)
            return n
        except ValueError:
            n += 1
        if n > 4 * num_frame + 4:
            raise AssertionError(f"no video length serves a {num_frame}-frame '{padding}' window")


def segment_mode(length: int, num_frame: int, padding: str) -> str:
    """The padding mode of a segment: the call's if the segment is long enough for it, "replicate" (any length >= 1) otherwise."""
    return padding if length >= min_length(num_frame, padding) else "replicate"


def scene_windows(n: int, cuts: Sequence[int], num_frame: int, padding: str) -> List[List[int]]:
    """Every frame's window of an n-frame video with the given cuts (video.window_lists when there are none and n is long enough)."""
    check_padding(padding)
    if n < 1:
        raise ValueError("the video has no frames")
    out = []
    for a, b in segments(n, check_cuts(cuts, n)):
        mode = segment_mode(b - a, num_frame, padding)
        out.extend([a + j for j in window_indices(i - a, b - a, num_frame, mode)] for i in range(a, b))
    return out


# ---- streaming ---------------------------------------------------------------------------------------------------------------------------
class ScenePlan:
    """What VideoUpscaler with cuts knows after each push: `seen` frames, the cuts among them, `done` frames returned.

    The segment of a frame is closed once a cut after it is known or the video has ended; its windows are then scene_windows'.  The last
    segment is open: it may end at any frame >= seen (a cut there, or the end of the video), so a frame of it is returned as soon as its
    window is the same for every such end, with the segment's mode following each candidate length.  A window never reaches back past its
    segment's start, so the frames to keep are bounded as without cuts: at most num_frame - 1 past frames (num_frame in the circle modes)."""

    def __init__(self, num_frame: int, padding: str):
        check_padding(padding)
        self.T, self.half, self.padding = num_frame, num_frame // 2, padding
        self.seen = 0
        self.done = 0
        self.cuts: List[int] = []
        self.ended = False

    def push(self, k: int, new_cuts: Sequence[int] = ()) -> None:
        """k more frames; new_cuts: the cuts among them (seen_before <= cut < seen_after, cut > 0), increasing."""
        lo, self.seen = self.seen, self.seen + k
        for c in new_cuts:
            if not (max(lo, 1) <= c < self.seen) or (self.cuts and c <= self.cuts[-1]):
                raise ValueError(f"cut {c} is not among frames {max(lo, 1)} .. {self.seen - 1} or repeats an earlier one")
            self.cuts.append(int(c))

    def end(self) -> None:
        self.ended = True

    def _segment(self, i: int) -> Tuple[int, Optional[int]]:
        """(start, end) of frame i's segment; end None while it is open."""
        p = bisect_right(self.cuts, i)
        a = self.cuts[p - 1] if p else 0
        if p < len(self.cuts):
            return a, self.cuts[p]
        return a, (self.seen if self.ended else None)

    def _lengths(self, r: int, l0: int) -> range:
        """The candidate lengths of an open segment that can give its frame r different windows: from l0 = the frames of it seen so
        far (at least r + 1) up to where the frame is interior on its right and the mode has settled; every longer one gives the last one's."""
        l0 = max(l0, r + 1)
        return range(l0, max(l0, r + self.half + 1, min_length(self.T, self.padding)) + 1)

    def window(self, i: int) -> Optional[List[int]]:
        """Frame i's window if it is settled, else None."""
        if not 0 <= i < self.seen:
            return None
        a, b = self._segment(i)
        if b is not None:
            return [a + j for j in window_indices(i - a, b - a, self.T, segment_mode(b - a, self.T, self.padding))]
        win = None
        for length in self._lengths(i - a, self.seen - a):
            w = window_indices(i - a, length, self.T, segment_mode(length, self.T, self.padding))
            if win is not None and w != win:
                return None
            win = w
        return [a + j for j in win]

    def take(self) -> List[List[int]]:
        """The windows of the frames that can be returned now, in order; they count as returned."""
        out = []
        while self.done < self.seen:
            w = self.window(self.done)
            if w is None:
                break
            out.append(w)
            self.done += 1
        return out

    def keep_from(self) -> int:
        """Oldest frame a window not returned yet may name, however the video continues."""
        lo = self.seen

        def reach(i: int, a: int, lengths) -> None:
            nonlocal lo
            for length in lengths:
                lo = min(lo, a + min(window_indices(i - a, length, self.T, segment_mode(length, self.T, self.padding))))

        for i in range(self.done, self.seen):
            a, b = self._segment(i)
            reach(i, a, (b - a,) if b is not None else self._lengths(i - a, self.seen - a))
        if not self.ended:          # frames to come: of the open segment, or of a later one, which names no frame seen so far;
            a = self.cuts[-1] if self.cuts else 0          # beyond seen + half a window starts after frame seen - half, which frame `seen` names
            for i in range(self.seen, self.seen + self.half + 1):
                reach(i, a, self._lengths(i - a, self.seen - a))
        return max(lo, 0)
