"""YUV4MPEG2 (.y4m) on any binary file object, non-seekable ones (pipes, stdin / stdout) included: the way to hand raw video to and
from another program (ffmpeg -f yuv4mpegpipe, x264, a player) without a library.

    YUV4MPEG2 W320 H180 F25:1 Ip A1:1 C420jpeg\\n          header: tags W H F I A C X, separated by single spaces
    FRAME\\n<h * w Y bytes><ch * cw U bytes><ch * cw V bytes>   per frame (an I420 frame, savsr_amd/yuv.py); FRAME may carry parameters

8-bit 4:2:0 only: C420, C420jpeg, C420mpeg2, C420paldv and a missing C tag (= 420) are read; every other tag is refused by name.  The
three 420 tags differ in chroma siting only: the reader hands it out as `siting` ("centre", "left", "topleft" of yuv.SITINGS, ffmpeg's
mapping of the three; None for a plain C420, a missing tag and every other tag, which carry none) and converts nothing itself; the
writer tags its output C420jpeg unless told another siting (Y4MWriter(..., siting=)).  XCOLORRANGE=FULL / XCOLORRANGE=LIMITED (ffmpeg's extension tag) is read into `colour_range` and written on
request; the format has no tag for the matrix (BT.601 / BT.709), which is the caller's to know or to guess from the frame size.

10 and 12 bits: Y4MReader(f, high_depth=True) also reads C420p10 and C420p12, whose frames hold little-endian 16-bit samples in the same
plane order (2 * i420_bytes bytes, still handed out as uint8 rows; `depth` says which).  The reader refuses them unless asked to, so that
a caller written against one byte per sample never receives two; Y4MWriter(..., depth=10 | 12) writes them.

4:2:2 and 4:4:4: Y4MReader(f, layouts=("420", "422", "444")) also reads C422 and C444, and with high_depth=True C422p10, C422p12, C444p10
and C444p12; `chroma` says which layout the stream has and `frame_bytes` is yuv.frame_bytes(height, width, depth, chroma).  An opt-in
like high_depth, for the same reason.  Y4MWriter(..., chroma="422" | "444") writes them.  These tags and the p10 / p12 ones name no
siting (`siting` is None): C422 means MPEG-2's horizontally cosited chroma to most tools, which is the caller's to say
(siting="left" of yuv.py).  C444alpha, Cmono, C411 and 14- / 16-bit tags stay refused by name.

Grey-scale: Y4MReader(f, mono=True) also reads Cmono, and with high_depth=True Cmono10 and Cmono12: `chroma` is "400" (yuv.MONO) and a
frame is the Y plane alone, yuv.frame_bytes(height, width, depth, "400") bytes.  An opt-in of its own, like high_depth, so every refusal
above keeps its words without it.  Y4MWriter(..., chroma="400") writes them.
"""
from __future__ import annotations

from fractions import Fraction
from typing import Iterator, Optional, Tuple

import numpy as np

from .yuv import CHROMAS, MONO, SITINGS, check_chroma, frame_bytes

MAGIC = b"YUV4MPEG2"
C420_TAGS = ("420", "420jpeg", "420mpeg2", "420paldv")
C420_SITINGS = {"420jpeg": "centre", "420mpeg2": "left", "420paldv": "topleft"}        # ffmpeg's reading of the three; no other tag names one
C420_HIGH_TAGS = {"420p10": 10, "420p12": 12}        # tag -> bit depth (Y4MReader with high_depth=True, Y4MWriter with depth=)
# 4:2:2 / 4:4:4 tags -> (chroma layout, bit depth); the high-depth ones need high_depth=True as well (Y4MReader with layouts=)
CHROMA_TAGS = {"422": ("422", 8), "444": ("444", 8)}
CHROMA_HIGH_TAGS = {f"{c}p{d}": (c, d) for c in ("422", "444") for d in (10, 12)}
MONO_TAGS = {"mono": 8}                              # grey-scale tag -> bit depth (Y4MReader with mono=True, Y4MWriter with chroma="400")
MONO_HIGH_TAGS = {"mono10": 10, "mono12": 12}        # (with high_depth=True as well)
MAX_LINE = 4096          # a header or FRAME line longer than this is not Y4M
COLOUR_RANGES = ("full", "limited")


def _ratio(tag: str, val: str) -> Tuple[int, int]:
    try:
        a, b = val.split(":")
        a, b = int(a), int(b)
    except ValueError:
        raise ValueError(f"y4m: bad header tag {tag}{val!r}: two integers a:b expected") from None
    if a < 0 or b < 0:
        raise ValueError(f"y4m: bad header tag {tag}{val!r}: two integers a:b expected")
    return a, b


def parse_fps(text: str) -> Tuple[int, int]:
    """'N' or 'N:D' -> (N, D), both positive."""
    try:
        n, _, d = text.partition(":")
        fps = (int(n), int(d) if d else 1)
    except ValueError:
        raise ValueError(f"frame rate {text!r}: N or N:D with positive integers expected") from None
    if fps[0] < 1 or fps[1] < 1:
        raise ValueError(f"frame rate {text!r}: N or N:D with positive integers expected")
    return fps


def scaled_aspect(aspect: Tuple[int, int], lr: Tuple[int, int], hr: Tuple[int, int]) -> Tuple[int, int]:
    """Pixel aspect a:b of the SR video such that the display aspect of the LR video is kept under an asymmetric scale:
    A' = Fraction(a * w * H, b * W * h), reduced, for LR (h, w) and HR (H, W).  0:0 (unknown) stays 0:0."""
    a, b = aspect
    if a == 0 or b == 0:
        return 0, 0
    (h, w), (H, W) = lr, hr
    f = Fraction(a * w * H, b * W * h)
    return f.numerator, f.denominator


def _read_exact(f, n: int) -> bytes:
    """Up to n bytes: fewer only at the end of the stream (a raw pipe returns what it has; keep reading)."""
    parts, got = [], 0
    while got < n:
        b = f.read(n - got)
        if not b:
            break
        parts.append(b)
        got += len(b)
    return parts[0] if len(parts) == 1 else b"".join(parts)


def _read_line(f) -> bytes:
    """One line including its newline, b"" at the end of the stream; byte by byte where the object has no readline."""
    if hasattr(f, "readline"):
        return f.readline(MAX_LINE)
    out = bytearray()
    while len(out) < MAX_LINE:
        b = f.read(1)
        if not b:
            break
        out += b
        if b == b"\n":
            break
    return bytes(out)


class Y4MReader:
    """Reads the header on construction (width, height, fps, interlace, aspect, colorspace, colour_range), then `chunks(k)` yields the
    frames as uint8 arrays [m, i420_bytes(height, width)], m = k but for the last.  colour_range: "full" / "limited" of an
    XCOLORRANGE=FULL / =LIMITED tag, None without one.  high_depth=True: C420p10 / C420p12 are read as well; `depth` is 8, 10 or 12 and
    the rows of a 10- or 12-bit stream are [m, 2 * i420_bytes(height, width)] uint8 (little-endian 16-bit samples).
    layouts: the chroma layouts (yuv.CHROMAS) the caller takes; with "422" / "444" in it C422 / C444 (and, with high_depth, their p10 /
    p12 forms) are read too, `chroma` is the stream's layout and the rows are [m, yuv.frame_bytes(height, width, depth, chroma)].
    The default reads 4:2:0 only and words every refusal as it did before layouts existed.
    siting (read-only): the chroma siting the C tag names, "centre" (C420jpeg), "left" (C420mpeg2) or "topleft" (C420paldv); None for
    a plain C420, a missing tag and every other tag.
    mono=True: Cmono (and, with high_depth, Cmono10 / Cmono12) is read as well: `chroma` is "400" and the rows are the Y planes alone,
    [m, yuv.frame_bytes(height, width, depth, "400")] uint8."""

    def __init__(self, f, high_depth: bool = False, layouts=("420",), mono: bool = False):
        self.f = f
        self.depth = 8
        self.chroma = "420"
        layouts = tuple(layouts)
        for c in layouts:
            check_chroma(c, "layouts")
        if "420" not in layouts:
            raise ValueError(f"y4m: layouts = {layouts!r} must include '420' (a stream without a C tag is 4:2:0)")
        more = tuple(c for c in CHROMAS if c in layouts and c != "420")
        line = _read_line(f)
        if not line.startswith(MAGIC + b" ") or not line.endswith(b"\n"):
            raise ValueError("y4m: not a YUV4MPEG2 stream (no 'YUV4MPEG2 ' header line)")
        self.width: Optional[int] = None
        self.height: Optional[int] = None
        self.fps: Tuple[int, int] = (25, 1)
        self.interlace = "p"
        self.aspect: Tuple[int, int] = (0, 0)
        self.colorspace = "420"
        self.colour_range: Optional[str] = None
        self._siting: Optional[str] = None
        for tag in line[len(MAGIC):].decode("ascii", errors="replace").split():
            key, val = tag[0], tag[1:]
            if key in "WH":
                try:
                    size = int(val)
                except ValueError:
                    size = 0
                if size < 1:
                    raise ValueError(f"y4m: bad header tag {tag!r}: a positive integer expected")
                if key == "W":
                    self.width = size
                else:
                    self.height = size
            elif key == "F":
                self.fps = _ratio("F", val)
            elif key == "I":
                self.interlace = val
            elif key == "A":
                self.aspect = _ratio("A", val)
            elif key == "C":
                if mono and (val in MONO_TAGS or (high_depth and val in MONO_HIGH_TAGS)):
                    self.chroma, self.depth = MONO, MONO_TAGS.get(val) or MONO_HIGH_TAGS[val]
                elif high_depth and val in C420_HIGH_TAGS:
                    self.depth, self.colorspace = C420_HIGH_TAGS[val], val
                elif val in CHROMA_TAGS and CHROMA_TAGS[val][0] in more:
                    self.chroma = CHROMA_TAGS[val][0]
                elif high_depth and val in CHROMA_HIGH_TAGS and CHROMA_HIGH_TAGS[val][0] in more:
                    self.chroma, self.depth = CHROMA_HIGH_TAGS[val]
                elif more and val not in C420_TAGS:
                    ok = C420_TAGS + (tuple(C420_HIGH_TAGS) if high_depth else ()) + more + \
                        (tuple(t for t, (c, _) in CHROMA_HIGH_TAGS.items() if c in more) if high_depth else ())
                    raise ValueError(f"y4m: colour space tag 'C{val}' is not supported: {', '.join('4:' + c[1] + ':' + c[2] for c in ('420',) + more)} "
                                     f"at {'8, 10 or 12 bits' if high_depth else '8 bits'} only ({', '.join('C' + t for t in ok)})")
                elif high_depth and val not in C420_TAGS:
                    raise ValueError(f"y4m: colour space tag 'C{val}' is not supported: 4:2:0 at 8, 10 or 12 bits only "
                                     f"({', '.join('C' + t for t in C420_TAGS + tuple(C420_HIGH_TAGS))})")
                elif val not in C420_TAGS:
                    raise ValueError(f"y4m: colour space tag 'C{val}' is not supported: 8-bit 4:2:0 only ({', '.join('C' + t for t in C420_TAGS)})")
                self.colorspace = val
                self._siting = C420_SITINGS.get(val)
            elif key == "X":                          # comments / extensions (XYSCSS=...): ignored, but for the range
                if val in ("COLORRANGE=FULL", "COLORRANGE=LIMITED"):
                    self.colour_range = val[11:].lower()
            else:
                raise ValueError(f"y4m: unknown header tag {tag!r}")
        if self.width is None or self.height is None:
            raise ValueError("y4m: the header names no W / H")
        self.frame_bytes = frame_bytes(self.height, self.width, self.depth, self.chroma)
        self.frames_read = 0

    @property
    def siting(self) -> Optional[str]:
        return self._siting

    def _frame_into(self, row: np.ndarray) -> bool:
        line = _read_line(self.f)
        if not line:
            return False
        i = self.frames_read
        if not (line.startswith(b"FRAME") and line.endswith(b"\n") and line[5:6] in (b" ", b"\n")):
            raise ValueError(f"y4m: frame {i}: 'FRAME' line expected, got {line[:16]!r}")
        data = _read_exact(self.f, self.frame_bytes)
        if len(data) != self.frame_bytes:
            raise ValueError(f"y4m: frame {i} is truncated: {len(data)} of {self.frame_bytes} bytes")
        row[:] = np.frombuffer(data, np.uint8)
        self.frames_read += 1
        return True

    def chunks(self, k: int) -> Iterator[np.ndarray]:
        if k < 1:
            raise ValueError("chunks of k >= 1 frames")
        while True:
            buf = np.empty((k, self.frame_bytes), np.uint8)
            m = 0
            while m < k and self._frame_into(buf[m]):
                m += 1
            if m:
                yield buf[:m]
            if m < k:
                return


class Y4MWriter:
    """Writes the header on construction, then `write(frames)` appends uint8 frames [m, i420_bytes(height, width)].
    colour_range = "full" / "limited": the header also carries XCOLORRANGE=FULL / =LIMITED (None: no such tag).  depth = 10, 12: the
    stream is tagged C420p10 / C420p12 and its frames are [m, 2 * i420_bytes(height, width)] uint8 (little-endian 16-bit samples).
    chroma = "422", "444": the stream is tagged C422 / C444 (C422p10 ... at depth 10 / 12) and its frames are
    [m, yuv.frame_bytes(height, width, depth, chroma)] uint8.  chroma = "400": grey-scale, tagged Cmono (Cmono10 / Cmono12), the frames
    are the Y planes alone.  siting: the chroma siting of the frames (yuv.SITINGS or None); an 8-bit
    4:2:0 stream is tagged C420mpeg2 for "left", C420paldv for "topleft" and C420jpeg otherwise; no other header has a tag for it."""

    def __init__(self, f, width: int, height: int, fps: Tuple[int, int] = (25, 1), interlace: str = "p", aspect: Tuple[int, int] = (0, 0),
                 colour_range: Optional[str] = None, depth: int = 8, chroma: str = "420", siting: Optional[str] = None):
        if width < 1 or height < 1:
            raise ValueError(f"y4m: W, H >= 1, got {width} x {height}")
        if colour_range is not None and colour_range not in COLOUR_RANGES:
            raise ValueError(f"y4m: colour_range = {colour_range!r}: None or one of {', '.join(COLOUR_RANGES)}")
        if depth != 8 and depth not in C420_HIGH_TAGS.values():
            raise ValueError(f"y4m: depth = {depth!r}: one of 8, 10, 12")
        try:
            if chroma != MONO:
                check_chroma(chroma)
        except ValueError as e:
            raise ValueError(f"y4m: {e}") from None
        if siting is not None and siting not in SITINGS:
            raise ValueError(f"y4m: siting = {siting!r}: None or one of {', '.join(SITINGS)}")
        self.f, self.width, self.height, self.depth, self.chroma = f, int(width), int(height), int(depth), chroma
        self.frame_bytes = frame_bytes(self.height, self.width, self.depth, chroma)
        tag420 = {"left": "420mpeg2", "topleft": "420paldv"}.get(siting, "420jpeg")
        ctag = (tag420 if chroma == "420" else chroma) if depth == 8 else f"{chroma}p{self.depth}"
        if chroma == MONO:
            ctag = "mono" if depth == 8 else f"mono{self.depth}"
        self.header = (f"YUV4MPEG2 W{self.width} H{self.height} F{fps[0]}:{fps[1]} I{interlace} A{aspect[0]}:{aspect[1]} C{ctag}"
                       f"{'' if colour_range is None else ' XCOLORRANGE=' + colour_range.upper()}\n").encode("ascii")
        f.write(self.header)

    def write(self, frames: np.ndarray) -> None:
        frames = np.ascontiguousarray(frames)
        if frames.dtype != np.uint8 or frames.ndim != 2 or frames.shape[1] != self.frame_bytes:
            raise ValueError(f"y4m: frames of {self.height} x {self.width} are [m, {self.frame_bytes}] uint8, got {frames.dtype} {tuple(frames.shape)}")
        for row in frames:
            self.f.write(b"FRAME\n")
            self.f.write(memoryview(row))
