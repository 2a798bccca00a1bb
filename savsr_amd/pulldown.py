"""Telecined film: inverse 3:2 pulldown, the host-side specification (numpy, integers only, no GPU needed).

Film at 24000/1001 frames/s is carried in 30000/1001 video by 3:2 pulldown: four film frames A B C D lie in five video frames as the
fields AA BB BC CD DD (`telecine` is that forward process).  Both fields of every film frame are in the stream, so the film can be
recovered exactly.  `pulldown=o` says "the video is telecined film with field order o"; the N video frames become N - N // cycle film
frames before anything else looks at them, and `upscale_video(v, pulldown=o, ...)` is, bit for bit,
`upscale_video(remove_pulldown(v, o, ...), ...)`.

"First field": the rows y with y % 2 == p, p = 0 for "tff" and 1 for "bff"; "second field": the rows of parity 1 - p.  Every rule works on
a matrix of R rows x C samples and only vertical neighbours meet, so packed [N, h, w, c] uint8 frames are the h x (w * c) byte matrix.

  1. Match (`field_scores`, `matches_from_scores`).  The second field of frame n is a temporal neighbour of its first field either in
     frame n - 1 or in frame n.  Candidate j = 0 takes it from frame max(n - 1, 0), j = 1 from frame n; a candidate's score is the sum
     over the second field's rows y, 1 <= y <= R - 2, and all x of |a - b| + |c - b| - |a - c|, a = F[n][y - 1], c = F[n][y + 1], b the
     candidate's sample at (y, x): twice the distance of b from the interval its vertical neighbours span.  It is 0 on a vertically
     monotone picture, positive where the fields comb, and an exact integer in any summation order.  delta[n] = -1 iff
     score[n, 0] < score[n, 1]; ties keep the frame's own field.  Keeping the first field makes the rule causal.
  2. Weave (`weave`).  Output frame n has the first-field rows of frame n and the second-field rows of frame max(n + delta[n], 0), in
     every plane; the chroma planes take the luma's parity, as savsr_amd/deinterlace.py does.  A byte copy at every depth.
  3. Decimate (`drops_from_sad`).  With sad[k] = scenes.pair_sad of woven frames k - 1, k (sad[0] counts as infinite), the frame with the
     smallest sad of every full cycle [cycle j, cycle j + cycle) is dropped, ties dropping the lowest index; a trailing partial cycle
     keeps all its frames.

How far ffmpeg is followed: the match is `fieldmatch`'s two-way (its "pc" mode) idea -- keep one field, choose the other between the
previous and the current frame -- with this project's own comb measure above, not fieldmatch's; the decimation is `decimate`'s rule
(drop the frame closest to its predecessor in each cycle) in exact integers over every sample pair_sad reads, without decimate's block
metrics or scene threshold.  ffmpeg is not available where this was written, so nothing here is pinned to its output.

  4. Clean (`comb_windows`, `combed_from_windows`; opt-in, `combed="yadif"` / `"bwdif"`).  Between the weave and the decimation every
     woven frame is measured for residual combing: a second-field sample (y, x), 1 <= y <= R - 2, is combed iff the match measure
     |a - b| + |c - b| - |a - c| of its own column exceeds 2 * comb_threshold; cells of 8 rows x 8 pixels anchored at (0, 0) count
     them, and a frame is flagged iff some 2 x 2 cell window (16 rows x 16 pixels, one at every cell origin, clipped at the edges, so
     windows overlap by half in both axes) holds at least comb_pixels of them.  A flagged frame is replaced by its same-rate
     deinterlaced form (savsr_amd/deinterlace.py, the temporal neighbours are the woven frames); the others pass as they are; the
     decimation sees the cleaned frames.  ffmpeg's fieldmatch -> yadif=deint=interlaced -> decimate chain is the idea; the defaults are
     fieldmatch's cthresh 9 and its combpel 80 of 256 rescaled to the 128 second-field samples of a window (40), and neither is
     validated on footage.

Limits.  There is no cadence tracking: every frame is matched and every cycle decimated on its own, so a cadence broken by an edit costs
one real frame in that cycle, as with decimate.  Without `combed=`, a leading frame whose partner field was cut off (a stream that starts
inside BC CD), the orphan field a broken cadence leaves and frames that match neither candidate -- video inserts -- stay combed
(`info["scores"]` has both candidates' scores); with it they are deinterlaced.  What remains with `combed=`: the decimation still drops
one of every `cycle` frames of a true-video insert (ffmpeg's constant-rate chain does too: judder, not combing); a cleaned frame has half
its rows interpolated; combing that is small (the two-pixel bar of the tests reads 32) or of low contrast stays below the rule; one
field order per video.  2:2 phase-shifted PAL film is not handled.  Nothing is validated on real footage or trained weights.
"""
from __future__ import annotations

from math import gcd
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .deinterlace import DEINTERLACERS, check_frame_rows, check_order, deinterlace_frames
from .frames import check_pixel_format, layout_of
from .scenes import pair_sad
from .yuv import MONO, check_depth, frame_bytes, layout_name, luma_plane, split_planes

CYCLE_MIN, CYCLE_MAX, DEFAULT_CYCLE = 2, 25, 5
DEFAULT_COMB_THRESHOLD, DEFAULT_COMB_PIXELS = 9, 40          # fieldmatch's cthresh; its combpel 80 / 256 of a window's 128 samples
COMB_CELL = 8                                                  # rows and pixels of a cell; a window is 2 x 2 cells
MAX_COMB_STEP = 4
FLOAT_REFUSAL = "float frames have no integer samples to deinterlace: give [N, h, w, c] uint8 or planar frames (quantise first)"


def check_cycle(cycle, what: str = "cycle") -> int:
    """The decimation cycle as an int: one frame in every `cycle` is dropped; 2 .. 25."""
    if isinstance(cycle, bool) or not isinstance(cycle, (int, np.integer)) or not CYCLE_MIN <= int(cycle) <= CYCLE_MAX:
        raise ValueError(f"{what} = {cycle!r}: an int in {CYCLE_MIN} .. {CYCLE_MAX}")
    return int(cycle)


def first_parity(order: str) -> int:
    """p: the first field is the rows y with y % 2 == p."""
    return check_order(order)


# ---- frames as planes ------------------------------------------------------------------------------------------------------------------------
def _as_numpy(frames) -> np.ndarray:
    if hasattr(frames, "detach"):
        frames = frames.detach().cpu().numpy()
    return np.asarray(frames)


def _frame_kind(frames: np.ndarray, pixel_format: str, size, depth: int):
    """(hw or None, layout or None, depth) of frames the pulldown rules take, after every check of them."""
    hw = check_pixel_format(pixel_format, size)
    if hw:
        h, w = hw
        layout, depth = layout_of(pixel_format), check_depth(depth)
        fb = frame_bytes(h, w, depth, layout)
        if frames.dtype != np.uint8 or frames.ndim != 2 or frames.shape[1] != fb:
            raise ValueError(f"{'' if depth == 8 else f'{depth}-bit '}{layout_name(layout)} frames of {h} x {w} are [N, {fb}] uint8, "
                             f"got {frames.dtype} {tuple(frames.shape)}")
        check_frame_rows(h, layout)
        return hw, layout, depth
    if depth != 8:
        raise ValueError(f"depth = {depth} goes with pixel_format = 'i420', 'i422', 'i444' or 'y400': packed frames are 8-bit")
    if frames.dtype.kind == "f":
        raise ValueError(FLOAT_REFUSAL)
    if frames.dtype != np.uint8 or frames.ndim != 4:
        raise ValueError(f"frames must be [N, h, w, c] uint8, got {frames.dtype} {tuple(frames.shape)}")
    check_frame_rows(frames.shape[1], None)
    return None, None, 8


def _planes(frames: np.ndarray, hw, layout, depth: int) -> List[np.ndarray]:
    """The [N, R, C] matrices of the frames: the byte matrix of packed frames, every plane of planar ones (the Y plane first)."""
    if not hw:
        n, h, w, c = frames.shape
        return [frames.reshape(n, h, w * c)]
    if layout == MONO:
        return [luma_plane(frames, hw[0], hw[1], depth, MONO)]
    return list(split_planes(frames, hw[0], hw[1], depth, layout))


def _join(planes: Sequence[np.ndarray], like: np.ndarray, hw, depth: int) -> np.ndarray:
    n = planes[0].shape[0]
    if not hw:
        return np.ascontiguousarray(planes[0]).reshape((n,) + like.shape[1:])
    return np.concatenate([np.ascontiguousarray(p.astype(np.uint8 if depth == 8 else "<u2")).reshape(n, -1).view(np.uint8) for p in planes], 1)


def _weave_matrix(m: np.ndarray, p: int, first, second) -> np.ndarray:
    res = m[first].copy()
    res[:, 1 - p::2] = m[second][:, 1 - p::2]
    return res


def weave_matrix(mats, order: str, delta: Sequence[int]) -> np.ndarray:
    """`weave` on [N, R, C] matrices of any R >= 1 (what savsr_video_weave does with one plane): the rows of parity p of matrix n, the
    others of matrix max(n + delta[n], 0)."""
    m = np.asarray(mats)
    n = m.shape[0]
    return _weave_matrix(m, first_parity(order), np.arange(n), np.maximum(np.arange(n) + np.asarray(delta, dtype=np.int64), 0))


def _weave_sources(frames, order: str, first: Sequence[int], second: Sequence[int], pixel_format: str, size, depth: int) -> np.ndarray:
    """Frame n of the result: the first-field rows of frames[first[n]] and the second-field rows of frames[second[n]], in every plane."""
    p = first_parity(order)
    frames = _as_numpy(frames)
    hw, layout, depth = _frame_kind(frames, pixel_format, size, depth)
    first, second = np.asarray(first, dtype=np.int64), np.asarray(second, dtype=np.int64)
    return _join([_weave_matrix(m, p, first, second) for m in _planes(frames, hw, layout, depth)], frames, hw, depth)


# ---- the rules -----------------------------------------------------------------------------------------------------------------------------------
def telecine_sources(n_film: int, phase: int = 0) -> Tuple[List[int], List[int]]:
    """(first, second): video frame n weaves the first field of film frame first[n] and the second field of film frame second[n]."""
    if isinstance(phase, bool) or not isinstance(phase, (int, np.integer)) or phase < 0:
        raise ValueError(f"phase = {phase!r}: a count of leading video frames to drop, >= 0")
    stream = [k for k in range(n_film) for _ in range(2 if k % 2 == 0 else 3)]          # the field stream alternates first / second
    pairs = [(stream[i], stream[i + 1]) for i in range(0, len(stream) - 1, 2)][int(phase):]          # (a trailing unpaired field is dropped)
    return [a for a, _ in pairs], [b for _, b in pairs]


def telecine(film, order: str, phase: int = 0, pixel_format: str = "rgb", size=None, depth: int = 8) -> np.ndarray:
    """The forward process, for tests and benchmarks: film frame k contributes 2 fields if k is even and 3 if it is odd, the field stream
    alternates first / second field and consecutive pairs are woven into frames (AA BB BC CD DD); a trailing unpaired field is dropped
    and `phase` drops that many leading video frames.  film: frames of any kind `weave` takes."""
    film = _as_numpy(film)
    first, second = telecine_sources(film.shape[0], phase)
    return _weave_sources(film, order, first, second, pixel_format, size, depth)


def field_scores(mats, order: str, depth: int = 8) -> np.ndarray:
    """[N, R, C] integer samples -> [N, 2] int64: score [n, j] of the module's docstring, j = 0 the second field of frame max(n - 1, 0),
    j = 1 frame n's own.  R < 3 gives zeros.  depth = 10 / 12: every sample is read as the 8 most significant bits of min(s, 2^depth - 1),
    as scenes.pair_sad reads it."""
    p = first_parity(order)
    m = np.asarray(mats)
    if m.ndim != 3 or m.dtype.kind not in "iu":
        raise ValueError(f"matrices must be [N, R, C] integers, got {m.dtype} {tuple(m.shape)}")
    depth = check_depth(depth)
    v = np.minimum(m.astype(np.int64), (1 << depth) - 1) >> (depth - 8)
    N, R, _ = v.shape
    out = np.zeros((N, 2), dtype=np.int64)
    ys = np.arange(1 - p, R, 2)
    ys = ys[(ys >= 1) & (ys <= R - 2)]
    if ys.size == 0:
        return out
    for n in range(N):
        a, c = v[n][ys - 1], v[n][ys + 1]
        for j, src in enumerate((max(n - 1, 0), n)):
            b = v[src][ys]
            out[n, j] = (np.abs(a - b) + np.abs(c - b) - np.abs(a - c)).sum(dtype=np.int64)
    return out


def frame_scores(frames, order: str, pixel_format: str = "rgb", size=None, depth: int = 8) -> np.ndarray:
    """`field_scores` of frames: every byte of packed [N, h, w, c] uint8 frames, the Y plane of planar ones."""
    check_order(order)
    frames = _as_numpy(frames)
    hw, layout, depth = _frame_kind(frames, pixel_format, size, depth)
    return field_scores(_planes(frames, hw, layout, depth)[0], order, depth)


def matches_from_scores(scores) -> List[int]:
    """delta[n] = -1 iff scores[n, 0] < scores[n, 1], else 0: ties keep the frame's own field."""
    return [-1 if int(s0) < int(s1) else 0 for s0, s1 in np.asarray(scores).reshape(-1, 2).tolist()]


def weave(frames, order: str, delta: Sequence[int], pixel_format: str = "rgb", size=None, depth: int = 8) -> np.ndarray:
    """Output frame n: the first-field rows of frame n and the second-field rows of frame max(n + delta[n], 0), in every plane."""
    frames = _as_numpy(frames)
    n = frames.shape[0]
    delta = [int(d) for d in delta]
    if len(delta) != n or any(d not in (-1, 0) for d in delta):
        raise ValueError(f"delta: one of -1, 0 per frame ({n} frames), got {delta!r}")
    return _weave_sources(frames, order, list(range(n)), [max(k + d, 0) for k, d in enumerate(delta)], pixel_format, size, depth)


def drops_from_sad(sad: Sequence[Optional[int]], cycle: int = DEFAULT_CYCLE, first: int = 0) -> List[int]:
    """The dropped frames among frames first .. first + len(sad) - 1 (`first` a multiple of cycle), from sad[k - first] = pair_sad of
    frames k - 1, k; the entry of frame 0 counts as infinite whatever it holds.  In every full cycle the frame with the smallest sad is
    dropped, ties dropping the lowest index; a trailing partial cycle keeps all its frames.  ffmpeg decimate's rule in exact integers."""
    cycle = check_cycle(cycle)
    if first % cycle:
        raise ValueError(f"first = {first}: a multiple of cycle = {cycle}")
    drops = []
    for c0 in range(0, len(sad) - cycle + 1, cycle):
        best = None
        for k in range(c0, c0 + cycle):
            if first + k == 0:
                continue
            if best is None or int(sad[k]) < int(sad[best]):
                best = k
        drops.append(first + best)
    return drops


def kept_from_drops(n: int, drops: Sequence[int]) -> List[int]:
    gone = set(drops)
    return [k for k in range(n) if k not in gone]


# ---- residual combing after the match ----------------------------------------------------------------------------------------------------------
def check_combed(combed, what: str = "combed") -> Optional[str]:
    """combed is None or a deinterlacer's name: how woven frames that are still combed are cleaned."""
    if combed is not None and combed not in DEINTERLACERS:
        raise ValueError(f"{what} = {combed!r}: None or one of {', '.join(repr(m) for m in DEINTERLACERS)}")
    return combed


def check_comb_threshold(threshold, what: str = "comb_threshold") -> int:
    """A sample is combed iff its measure exceeds 2 * threshold; an int in 0 .. 255 (the measure is at most 510)."""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, np.integer)) or not 0 <= int(threshold) <= 255:
        raise ValueError(f"{what} = {threshold!r}: an int in 0 .. 255")
    return int(threshold)


def check_comb_pixels(pixels, what: str = "comb_pixels") -> int:
    """A frame is combed iff a window holds this many combed pixels; an int in 1 .. 128 (a window has 128 second-field pixels)."""
    if isinstance(pixels, bool) or not isinstance(pixels, (int, np.integer)) or not 1 <= int(pixels) <= 2 * COMB_CELL * COMB_CELL:
        raise ValueError(f"{what} = {pixels!r}: an int in 1 .. {2 * COMB_CELL * COMB_CELL}")
    return int(pixels)


def check_comb_options(combed, comb_threshold, comb_pixels, have_match: bool, fields=None) -> Optional[str]:
    """combed= goes with pulldown= (or scan="detect") and not with fields=; comb_threshold= / comb_pixels= go with combed=."""
    if check_combed(combed) is None:
        for name, value, default in (("comb_threshold", comb_threshold, DEFAULT_COMB_THRESHOLD), ("comb_pixels", comb_pixels, DEFAULT_COMB_PIXELS)):
            if isinstance(value, bool) or value != default:
                raise ValueError(f"{name} = {value!r} goes with combed=: it is a parameter of the comb rule behind it")
        return None
    if fields is not None:
        raise ValueError(f"combed = {combed!r} together with fields = {fields!r}: fields= deinterlaces every frame; combed= cleans the frames "
                         f"the pulldown removal leaves combed and goes with pulldown=")
    if not have_match:
        raise ValueError(f"combed = {combed!r} goes with pulldown= (or scan='detect'): it cleans the frames the pulldown removal leaves combed")
    check_comb_threshold(comb_threshold)
    check_comb_pixels(comb_pixels)
    return combed


def comb_windows(mats, order: str, step: int = 1, threshold: int = DEFAULT_COMB_THRESHOLD, depth: int = 8) -> np.ndarray:
    """[N, R, C] integer samples -> [N, 2] int64: [n, 0] the largest count of combed samples in any window of matrix n, [n, 1] the count
    in the whole matrix.  A sample (y, x) on a second-field row, 1 <= y <= R - 2, is combed iff |a - b| + |c - b| - |a - c| >
    2 * threshold with a, b, c the samples at rows y - 1, y, y + 1 (read as `field_scores` reads them).  Cells are 8 rows x 8 * step
    samples anchored at (0, 0), clipped at the edges; a window is 2 x 2 cells, one at every cell origin, and counts what lies inside
    the matrix.  R < 3 gives zeros."""
    p = first_parity(order)
    m = np.asarray(mats)
    if m.ndim != 3 or m.dtype.kind not in "iu":
        raise ValueError(f"matrices must be [N, R, C] integers, got {m.dtype} {tuple(m.shape)}")
    if isinstance(step, bool) or not isinstance(step, (int, np.integer)) or not 1 <= int(step) <= MAX_COMB_STEP:
        raise ValueError(f"step = {step!r}: the samples of a pixel, 1 .. {MAX_COMB_STEP}")
    threshold, depth = check_comb_threshold(threshold, "threshold"), check_depth(depth)
    v = np.minimum(m.astype(np.int64), (1 << depth) - 1) >> (depth - 8)
    N, R, C = v.shape
    out = np.zeros((N, 2), dtype=np.int64)
    ys = np.arange(1 - p, R, 2)
    ys = ys[(ys >= 1) & (ys <= R - 2)]
    if ys.size == 0 or N == 0:
        return out
    a, b, c = v[:, ys - 1], v[:, ys], v[:, ys + 1]
    combed = (np.abs(a - b) + np.abs(c - b) - np.abs(a - c)) > 2 * threshold          # [N, len(ys), C]
    cw = COMB_CELL * int(step)
    ncr, ncc = -(-R // COMB_CELL), -(-C // cw)
    cells = np.zeros((N, ncr + 1, ncc + 1), dtype=np.int64)          # (one cell row and column of zeros: the clipped windows' far halves)
    rows_of = np.add.reduceat(combed.astype(np.int64), np.arange(0, C, cw), axis=2)          # [N, len(ys), ncc]
    np.add.at(cells, (slice(None), ys // COMB_CELL, slice(0, ncc)), rows_of)
    win = cells[:, :-1, :-1] + cells[:, 1:, :-1] + cells[:, :-1, 1:] + cells[:, 1:, 1:]
    out[:, 0] = win.reshape(N, -1).max(axis=1)
    out[:, 1] = cells.reshape(N, -1).sum(axis=1)
    return out


def frame_comb_windows(frames, order: str, pixel_format: str = "rgb", size=None, depth: int = 8, threshold: int = DEFAULT_COMB_THRESHOLD) -> np.ndarray:
    """`comb_windows` of frames: the byte matrix of packed [N, h, w, c] uint8 frames with step c, the Y plane of planar ones."""
    check_order(order)
    frames = _as_numpy(frames)
    hw, layout, depth = _frame_kind(frames, pixel_format, size, depth)
    return comb_windows(_planes(frames, hw, layout, depth)[0], order, 1 if hw else _comb_step(frames), threshold, depth)


def _comb_step(frames: np.ndarray) -> int:
    c = int(frames.shape[3])
    if not 1 <= c <= MAX_COMB_STEP:
        raise ValueError(f"frames have {c} channels: 1 .. {MAX_COMB_STEP}")
    return c


def combed_from_windows(win, step: int = 1, pixels: int = DEFAULT_COMB_PIXELS) -> List[bool]:
    """Frame n is combed iff its largest window count win[n, 0] reaches pixels * step (a pixel of packed frames is `step` samples)."""
    return [int(w0) >= int(pixels) * int(step) for w0 in np.asarray(win).reshape(-1, 2)[:, 0].tolist()]


def clean_combed(woven, order: str, flags: Sequence[bool], method: str, pixel_format: str = "rgb", size=None, depth: int = 8) -> np.ndarray:
    """The woven frames with every flagged one replaced by frame n of deinterlace_frames(woven, ..., method, rate="same"): its temporal
    neighbours are woven frames, not cleaned ones; every plane is cleaned."""
    woven = _as_numpy(woven)
    if not any(flags):
        return woven.copy()
    clean = deinterlace_frames(woven, order, pixel_format, size, depth, method, "same")
    out = woven.copy()
    idx = [k for k, f in enumerate(flags) if f]
    out[idx] = clean[idx]
    return out


def remove_pulldown_frames(frames, order: str, pixel_format: str = "rgb", size=None, depth: int = 8, cycle: int = DEFAULT_CYCLE, combed=None,
                           comb_threshold: int = DEFAULT_COMB_THRESHOLD, comb_pixels: int = DEFAULT_COMB_PIXELS) -> Tuple[np.ndarray, Dict[str, object]]:
    """The film frames of a telecined video, in the same format, and info = {"scores": int64 [N, 2], "matches": [N] of -1 | 0, "sad":
    int64 [N] (pair_sad of the woven frames k - 1, k; entry 0 is -1 and counts as infinite), "kept": the indices of the kept woven
    frames}: the composition of the rules above.  frames: [N, h, w, c] uint8, or with pixel_format "i420", "i422", "i444", "y400" and
    size=(h, w): [N, frame_bytes] uint8, little-endian 16-bit samples at depth 10 / 12.  Float frames are refused.  combed="yadif" /
    "bwdif": woven frames that `comb_windows` / `combed_from_windows` (comb_threshold, comb_pixels) flag are deinterlaced at same rate
    before the decimation, which then reads the cleaned frames; info gains "comb" (int64 [N, 2]) and "combed" (the flagged woven
    indices)."""
    check_order(order)
    cycle = check_cycle(cycle)
    check_comb_options(combed, comb_threshold, comb_pixels, True)
    frames = _as_numpy(frames)
    hw = _frame_kind(frames, pixel_format, size, depth)[0]
    n = frames.shape[0]
    if n < 1:
        raise ValueError("the video has no frames")
    scores = frame_scores(frames, order, pixel_format, size, depth)
    matches = matches_from_scores(scores)
    woven = weave(frames, order, matches, pixel_format, size, depth)
    extra = {}
    if combed is not None:
        win = frame_comb_windows(woven, order, pixel_format, size, depth, comb_threshold)
        flags = combed_from_windows(win, 1 if hw else _comb_step(frames), comb_pixels)
        woven = clean_combed(woven, order, flags, combed, pixel_format, size, depth)
        extra = {"comb": win, "combed": [k for k, f in enumerate(flags) if f]}
    sad = np.concatenate([np.array([-1], dtype=np.int64), pair_sad(woven, pixel_format, size, depth)])
    kept = kept_from_drops(n, drops_from_sad(sad.tolist(), cycle))
    return woven[kept], {"scores": scores, "matches": matches, "sad": sad, "kept": kept, **extra}


# ---- the command line's header decision --------------------------------------------------------------------------------------------------------
PULLDOWN_FLAGS = ("none", "auto", "tff", "bff")


def film_rate(fps: Tuple[int, int], cycle: int = DEFAULT_CYCLE) -> Tuple[int, int]:
    """fps * (cycle - 1) / cycle as a reduced integer pair: 30000/1001 -> 24000/1001."""
    a, b = int(fps[0]) * (cycle - 1), int(fps[1]) * cycle
    g = gcd(a, b) or 1
    return a // g, b // g


def resolve_pulldown(flag: Optional[str], tag: Optional[str], fps: Tuple[int, int], cycle: int = DEFAULT_CYCLE):
    """--pulldown and the input's interlace tag -> (order or None, the output's interlace tag, the output's frame rate, a note for stderr
    or None).  flag: one of PULLDOWN_FLAGS, or None when --pulldown was not given; tag: the Y4M input's I tag, None for a PNG folder.
    Without pulldown removal the tag and the rate pass through; with it the output is progressive at fps * (cycle - 1) / cycle.
    auto reads the tag as --fields auto does: It -> tff, Ib -> bff, Ip -> nothing to do; Im (mixed) and a PNG folder are refused."""
    if flag is not None and flag not in PULLDOWN_FLAGS:
        raise ValueError(f"--pulldown = {flag!r}: one of {', '.join(PULLDOWN_FLAGS)}")
    cycle = check_cycle(cycle, "--pulldown-cycle")
    keep = "p" if tag is None else tag
    same = (int(fps[0]), int(fps[1]))
    if flag is None or flag == "none":
        if cycle != DEFAULT_CYCLE:
            raise ValueError(f"--pulldown-cycle = {cycle} goes with --pulldown: it is the decimation cycle of the pulldown removal")
        return None, keep, same, None
    if flag == "auto":
        if tag is None:
            raise ValueError("--pulldown auto reads the Y4M input's I tag; a PNG folder has none: give --pulldown tff or --pulldown bff")
        if tag == "m":
            raise ValueError("--pulldown auto: the input is tagged Im (mixed progressive and interlaced frames), which is not modelled; give "
                             "--pulldown tff or --pulldown bff to treat every frame as telecined film")
        if tag not in ("t", "b"):
            return None, keep, same, "--pulldown auto: the input is not tagged interlaced, so there are no fields to match: nothing is removed"
        order = "tff" if tag == "t" else "bff"
    else:
        order = flag
    return order, "p", film_rate(fps, cycle), None
