"""Video surfaces: where the samples of a frame lie in memory, when that is not the tightly packed planar frame of a Y4M file.

`pixel_format`, `depth` and `size` say which samples a frame has; a `Surface` says where they lie.  Hardware decoders hand out
semi-planar surfaces (NV12, P010) with a row pitch and padded line counts, capture cards packed 4:2:2 (UYVY, YUYV), software decoders
planar frames whose `linesize` is wider than the picture.  One HIP kernel pair at the boundary (csrc/surface.hip, `prepass.unpack_surface`
/ `pack_surface`) converts any of them to the project's planar frames and back; everything between works on planar frames as ever.

A surface is one to three *surface planes*.  A surface plane is a pitched byte matrix that holds `step` interleaved component streams;
stream k names the planar plane it carries (0 = Y, 1 = U, 2 = V) and which sample of that plane's row group g holds: `mul * g + add`.

    pitched planar                       three planes (one for "400"), step 1
    NV12 / NV21 / NV16, P010 / P012 /    the Y plane, step 1, then one chroma plane, step 2, carrying [U, V] ([V, U] for NV21);
    P210 / P212                          the P formats are 16-bit words with the sample in their high `depth` bits (msb)
    UYVY / YUYV                          one plane, step 4: [U, Y(2g), V, Y(2g + 1)] / [Y(2g), U, Y(2g + 1), V]

This module is the specification, in integers: `Surface.resolve` gives the concrete table for a frame size, `unpack_frames` and
`pack_frames` are what the kernels equal bit for bit.  Host only: numpy, no library.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple, Optional, Tuple

import numpy as np

from .yuv import DEPTHS, MONO, chroma_hw, frame_bytes, layout_name

LAYOUTS = ("420", "422", "444", MONO)
_BLOCK = {"420": (2, 2), "422": (1, 2), "444": (1, 1), MONO: (1, 1)}          # (vertical, horizontal) chroma block

# kind -> (the layouts it admits, the depths it admits, msb, the plane shape: "planar" | "semi" | "packed", the stream order)
# stream order: semi: the planar planes of the chroma plane's two streams; packed: per byte of a group (plane, mul, add)
_KINDS = {
    "planar": (LAYOUTS, DEPTHS, None, "planar", None),
    "nv12": (("420",), (8,), False, "semi", (1, 2)),
    "nv21": (("420",), (8,), False, "semi", (2, 1)),
    "nv16": (("422",), (8,), False, "semi", (1, 2)),
    "p010": (("420",), (10,), True, "semi", (1, 2)),
    "p012": (("420",), (12,), True, "semi", (1, 2)),
    "p210": (("422",), (10,), True, "semi", (1, 2)),
    "p212": (("422",), (12,), True, "semi", (1, 2)),
    "uyvy": (("422",), (8,), False, "packed", ((1, 1, 0), (0, 2, 0), (2, 1, 0), (0, 2, 1))),
    "yuyv": (("422",), (8,), False, "packed", ((0, 2, 0), (1, 1, 0), (0, 2, 1), (2, 1, 0))),
}
KINDS = tuple(_KINDS)


class Stream(NamedTuple):
    """One component stream of a surface plane: group g holds sample `mul * g + add` of a row of planar plane `plane` (0 Y, 1 U, 2 V);
    a group whose sample lies past the row's end is padding (the second Y of an odd-width packed row)."""
    plane: int
    mul: int
    add: int


class SurfacePlane(NamedTuple):
    """A pitched byte matrix of a surface, `offset` bytes into the frame: `rows` rows of `groups` groups of len(streams) samples,
    rows `pitch` bytes apart."""
    offset: int
    pitch: int
    rows: int
    groups: int
    streams: Tuple[Stream, ...]

    @property
    def step(self) -> int:
        return len(self.streams)


class SurfaceTable(NamedTuple):
    """A surface at a frame size: the bytes of a frame (the whole allocation, padded lines included), the sample size in bytes, whether
    16-bit words carry the sample in their high `depth` bits, the depth, and the surface planes."""
    bytes: int
    sample: int
    msb: bool
    depth: int
    planes: Tuple[SurfacePlane, ...]

    def row_bytes(self, p: SurfacePlane) -> int:
        return p.groups * p.step * self.sample

    @property
    def span(self) -> int:
        """One past the last byte that holds a sample."""
        return max(p.offset + (p.rows - 1) * p.pitch + self.row_bytes(p) for p in self.planes)

    @property
    def tight(self) -> bool:
        """Every byte of the frame lies in a row of a plane (no row padding, no padded lines)."""
        return sum(p.rows * self.row_bytes(p) for p in self.planes) == self.bytes


def _round_up(v: int, a: int) -> int:
    return -(-v // a) * a


def _pos_int(v, what: str, low: int = 1) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < low:
        raise ValueError(f"{what} = {v!r}: an int >= {low}")
    return int(v)


@dataclass(frozen=True)
class Surface:
    """The memory layout of a frame, before its size is known: a kind (`KINDS`) and either explicit `pitch` / `lines` or `pitch_align` /
    `lines_align`.  pitch: bytes per row of the first plane (the chroma plane of semi-planar surfaces shares it); lines: allocated rows of
    the first plane; the following planes start at pitch * lines, as decoders lay them out, unless `offsets` names every plane's start.
    chroma_pitch (pitched planar only): bytes per row of the U and V planes, default the luma pitch divided by the horizontal chroma
    block, rounded up to the sample size.  msb: 16-bit words carry the sample in their high `depth` bits.  The default is tight rows
    and no padding.  Build one with the named constructors; `resolve(h, w, depth, layout)` gives the table or refuses by name."""
    kind: str
    pitch: Optional[int] = None
    lines: Optional[int] = None
    chroma_pitch: Optional[int] = None
    pitch_align: int = 1
    lines_align: int = 1
    offsets: Optional[Tuple[int, ...]] = None
    msb: bool = False

    def __post_init__(self):
        if self.kind not in _KINDS:
            raise ValueError(f"surface kind = {self.kind!r}: one of {', '.join(KINDS)}")
        for what in ("pitch", "lines", "chroma_pitch"):
            if getattr(self, what) is not None:
                object.__setattr__(self, what, _pos_int(getattr(self, what), what))
        for what, explicit in (("pitch_align", self.pitch), ("lines_align", self.lines)):
            a = _pos_int(getattr(self, what), what)
            if a != 1 and explicit is not None:
                raise ValueError(f"{what} = {a} together with {what[:-6]} = {explicit}: give the {what[:-6]} or its alignment, not both")
        if self.chroma_pitch is not None and self.kind != "planar":
            raise ValueError(f"chroma_pitch goes with Surface.planar(): the chroma plane of {self.kind} shares the luma pitch")
        if self.offsets is not None:
            object.__setattr__(self, "offsets", tuple(_pos_int(o, "offsets[]", 0) for o in self.offsets))
        if not isinstance(self.msb, bool):
            raise ValueError(f"msb = {self.msb!r}: True or False")

    # ---- the named constructors --------------------------------------------------------------------------------------------------------
    @classmethod
    def _make(cls, kind, pitch, lines, chroma_pitch=None, pitch_align=1, lines_align=1, offsets=None, msb=None) -> "Surface":
        return cls(kind, pitch, lines, chroma_pitch, pitch_align, lines_align, offsets, bool(_KINDS[kind][2]) if msb is None else msb)

    @classmethod
    def planar(cls, pitch=None, lines=None, chroma_pitch=None, *, pitch_align=1, lines_align=1, offsets=None, msb=False) -> "Surface":
        """Planar frames with a row pitch (a software decoder's `linesize`): Y, then U and V."""
        return cls._make("planar", pitch, lines, chroma_pitch, pitch_align, lines_align, offsets, msb)

    def resolve(self, h: int, w: int, depth: int = 8, layout: str = "420") -> SurfaceTable:
        """The concrete table of this surface for h x w frames of `depth` bits in chroma layout `layout` ("420", "422", "444", "400");
        refuses, by name, what cannot be: a pitch below the row's bytes, lines below h, an odd pitch or offset with 16-bit samples, msb
        at depth 8, a constructor of another layout or depth, overlapping planes."""
        layouts, depths, _, shape, order = _KINDS[self.kind]
        h, w = _pos_int(h, "h"), _pos_int(w, "w")
        if layout not in LAYOUTS:
            raise ValueError(f"layout = {layout!r}: one of {', '.join(LAYOUTS)}")
        if depth not in DEPTHS:
            raise ValueError(f"depth = {depth!r}: one of {', '.join(str(d) for d in DEPTHS)}")
        name = f"Surface.{self.kind}()"
        if layout not in layouts:
            raise ValueError(f"{name} holds {' / '.join(layout_name(c) for c in layouts)} samples, the frames are {layout_name(layout)}")
        if depth not in depths:
            raise ValueError(f"{name} holds {' / '.join(str(d) for d in depths)}-bit samples, the frames have depth = {depth}")
        if self.msb and depth == 8:
            raise ValueError("msb = True at depth 8: only 16-bit words (depth 10, 12) have high bits to carry the sample in")
        s = 1 if depth == 8 else 2
        mono = layout == MONO
        ch, cw = (0, 0) if mono else chroma_hw(h, w, layout)
        bv, bh = _BLOCK[layout]
        # the planes as (rows, groups, streams, which pitch: 0 luma / 1 chroma, vertical block of the allocated lines)
        if shape == "planar":
            shapes = [(h, w, (Stream(0, 1, 0),), 0, 1)]
            if not mono:
                shapes += [(ch, cw, (Stream(1, 1, 0),), 1, bv), (ch, cw, (Stream(2, 1, 0),), 1, bv)]
        elif shape == "semi":
            shapes = [(h, w, (Stream(0, 1, 0),), 0, 1), (ch, cw, (Stream(order[0], 1, 0), Stream(order[1], 1, 0)), 0, bv)]
        else:
            shapes = [(h, cw, tuple(Stream(*t) for t in order), 0, 1)]
        row_bytes = [groups * len(streams) * s for _, groups, streams, _, _ in shapes]
        if self.pitch is not None:
            pitch = self.pitch
        else:          # the rows that share the first pitch all fit: an odd-width NV12 row has 2 * ceil(w / 2) chroma samples
            pitch = _round_up(max(rb for rb, sh in zip(row_bytes, shapes) if sh[3] == 0), self.pitch_align)
        lines = self.lines if self.lines is not None else _round_up(h, self.lines_align)
        if self.chroma_pitch is not None:
            cpitch = self.chroma_pitch
        else:
            cpitch = _round_up(-(-pitch // bh), s)
        if lines < h:
            raise ValueError(f"lines = {lines} below the frame's {h} rows")
        offsets, end = [], 0
        for k, (rows, groups, streams, which, vb) in enumerate(shapes):
            p = cpitch if which else pitch
            what = "chroma_pitch" if which else "pitch"
            if p < row_bytes[k]:
                odd = "; a chroma row of odd width w has 2 * ceil(w / 2) samples" if len(streams) == 2 and w % 2 else ""
                raise ValueError(f"{what} = {p} below the {row_bytes[k]} bytes of a row of plane {k} ({groups * len(streams)} samples of "
                                 f"{s} byte{'s' if s > 1 else ''}{odd})")
            if s == 2 and p % 2:
                raise ValueError(f"{what} = {p} is odd: {depth}-bit samples are 16-bit words")
            offsets.append(end)
            end += p * -(-lines // vb)
        if self.offsets is not None:
            if len(self.offsets) != len(shapes):
                raise ValueError(f"offsets = {self.offsets}: {name} of {layout_name(layout)} frames has {len(shapes)} "
                                 f"plane{'s' if len(shapes) > 1 else ''}")
            offsets = list(self.offsets)
        planes = []
        for k, (rows, groups, streams, which, vb) in enumerate(shapes):
            if s == 2 and offsets[k] % 2:
                raise ValueError(f"offset {offsets[k]} of plane {k} is odd: {depth}-bit samples are 16-bit words")
            planes.append(SurfacePlane(offsets[k], cpitch if which else pitch, rows, groups, streams))
        total = max(p.offset + p.pitch * -(-lines // sh[4]) for p, sh in zip(planes, shapes))
        tab = SurfaceTable(total, s, bool(self.msb), depth, tuple(planes))
        ext = sorted((p.offset, p.offset + (p.rows - 1) * p.pitch + tab.row_bytes(p), k) for k, p in enumerate(planes))
        for (a0, a1, ka), (b0, b1, kb) in zip(ext, ext[1:]):
            if b0 < a1:
                raise ValueError(f"planes {ka} and {kb} overlap: bytes [{a0}, {a1}) and [{b0}, {b1})")
        return tab


def _named(kind: str):
    def make(cls, pitch=None, lines=None, *, pitch_align=1, lines_align=1, offsets=None) -> Surface:
        return cls._make(kind, pitch, lines, None, pitch_align, lines_align, offsets)
    make.__name__ = kind
    make.__doc__ = {"semi": "Semi-planar {0}: the Y plane, then one plane of interleaved chroma pairs.",
                    "packed": "Packed 8-bit 4:2:2 {0}: one plane of four-byte groups."}[_KINDS[kind][3]].format(kind.upper())
    return classmethod(make)


for _k in KINDS[1:]:
    setattr(Surface, _k, _named(_k))


def check_surface(surface, what: str = "surface") -> Surface:
    if not isinstance(surface, Surface):
        raise TypeError(f"{what} must be a savsr_amd.surface.Surface (Surface.nv12(), Surface.planar(pitch=...), ...), got {type(surface).__name__}")
    return surface


def check_stride(stride: int, tab: SurfaceTable, what: str = "frames") -> None:
    """The frame stride of surface frames may exceed the surface's bytes (decoders pad frames too), never fall below them."""
    if stride < tab.bytes:
        raise ValueError(f"{what} have a frame stride of {stride} bytes, the surface takes {tab.bytes}")
    if tab.sample == 2 and stride % 2:
        raise ValueError(f"{what} have an odd frame stride of {stride} bytes: {tab.depth}-bit samples are 16-bit words")


def planar_planes(h: int, w: int, depth: int, layout: str):
    """(offset, rows, cols) in samples of the Y, U, V planes of a planar frame (Y alone for "400")."""
    planes = [(0, h, w)]
    if layout != MONO:
        ch, cw = chroma_hw(h, w, layout)
        planes += [(h * w, ch, cw), (h * w + ch * cw, ch, cw)]
    return planes


def _byte_index(tab: SurfaceTable, p: SurfacePlane, k: int):
    """[rows, groups] byte offsets into a surface frame of stream k's samples."""
    return p.offset + np.arange(p.rows, dtype=np.int64)[:, None] * p.pitch + (np.arange(p.groups, dtype=np.int64)[None, :] * p.step + k) * tab.sample


def _check_frames(frames, what: str) -> np.ndarray:
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 2:
        raise ValueError(f"{what} must be [N, bytes] uint8, got {frames.dtype} {frames.shape}")
    return frames


def unpack_frames(frames, surface: Surface, h: int, w: int, depth: int = 8, layout: str = "420") -> np.ndarray:
    """Surface frames [N, stride] uint8 -> planar frames [N, frame_bytes(h, w, depth, layout)] uint8.  An msb word x becomes
    x >> (16 - depth); other samples are copied verbatim.  Bytes no sample maps to are not read."""
    tab = check_surface(surface).resolve(h, w, depth, layout)
    frames = _check_frames(frames, "surface frames")
    check_stride(frames.shape[1], tab)
    n = frames.shape[0]
    pl = planar_planes(h, w, depth, layout)
    mats = [np.zeros((n, rows, cols), dtype=np.uint16 if tab.sample == 2 else np.uint8) for _, rows, cols in pl]
    for p in tab.planes:
        for k, st in enumerate(p.streams):
            off, rows, cols = pl[st.plane]
            x = st.mul * np.arange(p.groups) + st.add
            keep = x < cols
            idx = _byte_index(tab, p, k)[:, keep]
            v = frames[:, idx]
            if tab.sample == 2:
                v = v.astype(np.uint16) | (frames[:, idx + 1].astype(np.uint16) << 8)
                if tab.msb:
                    v = v >> (16 - depth)
            mats[st.plane][:, :, x[keep]] = v
    out = np.concatenate([m.reshape(n, -1) for m in mats], 1)
    assert out.shape[1] * tab.sample == frame_bytes(h, w, depth, layout)
    return out.astype("<u2").view(np.uint8).reshape(n, -1) if tab.sample == 2 else out


def pack_frames(planar, surface: Surface, h: int, w: int, depth: int = 8, layout: str = "420") -> np.ndarray:
    """Planar frames [N, frame_bytes(h, w, depth, layout)] uint8 -> surface frames [N, surface bytes] uint8 in which every byte no
    sample maps to is 0: row padding, padded lines, the low bits of msb words, the pad Y of an odd-width packed row.  An msb sample s
    is written as min(s, 2^depth - 1) << (16 - depth); other samples are copied verbatim."""
    tab = check_surface(surface).resolve(h, w, depth, layout)
    planar = _check_frames(planar, "planar frames")
    fb = frame_bytes(h, w, depth, layout)
    if planar.shape[1] != fb:
        raise ValueError(f"{'' if depth == 8 else f'{depth}-bit '}{layout_name(layout)} frames of {h} x {w} have {fb} bytes, got {planar.shape[1]}")
    n = planar.shape[0]
    src = np.ascontiguousarray(planar).view("<u2").astype(np.uint16) if tab.sample == 2 else planar
    out = np.zeros((n, tab.bytes), dtype=np.uint8)
    pl = planar_planes(h, w, depth, layout)
    for p in tab.planes:
        for k, st in enumerate(p.streams):
            off, rows, cols = pl[st.plane]
            x = st.mul * np.arange(p.groups) + st.add
            keep = x < cols
            idx = _byte_index(tab, p, k)[:, keep]
            v = src[:, off:off + rows * cols].reshape(n, rows, cols)[:, :, x[keep]]
            if tab.sample == 2:
                if tab.msb:
                    v = np.minimum(v, (1 << depth) - 1).astype(np.uint16) << (16 - depth)
                out[:, idx] = (v & 255).astype(np.uint8)
                out[:, idx + 1] = (v >> 8).astype(np.uint8)
            else:
                out[:, idx] = v
    return out


def descriptor(tab: SurfaceTable) -> np.ndarray:
    """The table as the int64 words the C ABI takes (savsr_video_unpack_surface / _pack_surface): per plane offset, pitch, rows, groups,
    step, then (plane, mul, add) of four streams (unused ones 0)."""
    d = np.zeros((len(tab.planes), 17), dtype=np.int64)
    for i, p in enumerate(tab.planes):
        d[i, :5] = (p.offset, p.pitch, p.rows, p.groups, p.step)
        for k, st in enumerate(p.streams):
            d[i, 5 + 3 * k:8 + 3 * k] = st
    return d
