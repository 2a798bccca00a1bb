"""The frames of a video call, by name and without device work: the format names, the argument checks, `Side` and `VideoSpec`, and
the plane table -- where the byte matrices of a frame lie inside it.  Everything here runs on the host and loads no library; the
specification modules (scenes.py, active.py, deinterlace.py, pulldown.py), the device stages (prepass.py) and the sequence path
(video.py, whose module text says what a `VideoSpec` is for) all import it, and it imports none of them.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple, Optional, Tuple

import torch

from .dither import check_dither
from .harness import window_indices
from .yuv import (CHROMA_OF, LUMA_FORMAT, MONO, check_chroma_filter, check_colour, check_depth, check_depth_colour, check_siting, chroma_hw, frame_bytes,
                  layout_name)

PADDING_MODES = ("replicate", "reflection", "reflection_circle", "circle")
OUT_KINDS = ("float", "uint8", "i420", "i422", "i444")
PIXEL_FORMATS = ("rgb", "i420", "i422", "i444")
YUV_FORMATS = ("i420", "i422", "i444")          # planar YUV in the three chroma layouts (yuv.CHROMAS), as pixel_format and as out
# "y400": grey-scale frames, the Y plane alone, for luma-only networks; accepted beside the two lists above, which stay as they were
SAMPLE_FORMATS = YUV_FORMATS + (LUMA_FORMAT,)   # frames of planar samples with a bit depth
_YUV_LIST = "'i420', 'i422' or 'i444'"


def chroma_of(fmt: str) -> str:
    """The chroma layout ("420", "422", "444") of a YUV pixel format / output kind; "420" for the others (no YUV on that side)."""
    return CHROMA_OF.get(fmt, "420")


def layout_of(fmt: str) -> str:
    """chroma_of, with yuv.MONO ("400") for grey-scale frames ("y400")."""
    return MONO if fmt == LUMA_FORMAT else chroma_of(fmt)


def as_scale(scale) -> Tuple[float, float]:
    """A float (symmetric) or an (sh, sw) pair -> (sh, sw) floats."""
    if isinstance(scale, (int, float)) and not isinstance(scale, bool):
        sc = (float(scale), float(scale))
    else:
        try:
            sh, sw = scale
            sc = (float(sh), float(sw))
        except (TypeError, ValueError):
            raise ValueError(f"scale must be a number or an (sh, sw) pair, got {scale!r}") from None
    if not (sc[0] > 0 and sc[1] > 0):
        raise ValueError(f"scale must be positive, got {sc}")
    return sc


def check_padding(padding: str) -> None:
    if padding not in PADDING_MODES:
        raise ValueError(f"padding = {padding!r} is not a mode of generate_frame_indices: one of {', '.join(PADDING_MODES)}")


def check_length(n: int, num_frame: int, padding: str) -> None:
    """Every frame's window lies inside the video (the refusal of datasets.py for a too-short folder, in the same words)."""
    if n < 1:
        raise ValueError("the video has no frames")
    for i in range(n):
        win = window_indices(i, n, num_frame, padding)
        if min(win) < 0 or max(win) >= n:
            raise ValueError(f"video has {n} frames: too few for a {num_frame}-frame '{padding}' window")


def _packed_dims(frames: torch.Tensor) -> Tuple[int, int, int, int]:
    """(N, c, h, w) of a packed video tensor: [N, h, w, c] uint8 (GPU or host) or [N, c, h, w] float on the GPU; refuses anything else."""
    if frames.dim() != 4:
        raise ValueError(f"frames must be [N, h, w, c] uint8 or [N, c, h, w] float, got {frames.dim()} dimensions")
    if frames.dtype == torch.uint8:
        n, h, w, c = frames.shape
    elif frames.is_floating_point():
        if not frames.is_cuda:
            raise ValueError("float frames must be on the GPU ([N, c, h, w]); host frames go as [N, h, w, c] uint8")
        n, c, h, w = frames.shape
    else:
        raise ValueError(f"frames must be uint8 or float, got {frames.dtype}")
    return int(n), int(c), int(h), int(w)


def frame_layout(frames: torch.Tensor, nch: int) -> Tuple[int, int, int]:
    """(N, h, w) of a packed video tensor (`_packed_dims`) of the network's nch channels and at least 2 x 2."""
    if not isinstance(frames, torch.Tensor):
        raise TypeError(f"frames must be a torch.Tensor, got {type(frames).__name__}")
    n, c, h, w = _packed_dims(frames)
    if c != nch:
        raise ValueError(f"frames have {c} channels, the network takes num_in_ch = {nch}")
    if h < 2 or w < 2:
        raise ValueError(f"SAVSR needs h, w >= 2, got {h} x {w}")
    return n, h, w


def check_pixel_format(pixel_format: str, size) -> Optional[Tuple[int, int]]:
    """(h, w) of YUV frames (i420, i422, i444), None for RGB ones; refuses an unknown format, YUV without a size and a size without YUV."""
    if pixel_format not in PIXEL_FORMATS and pixel_format != LUMA_FORMAT:
        raise ValueError(f"pixel_format = {pixel_format!r}: one of {', '.join(PIXEL_FORMATS)}")
    if pixel_format == "rgb":
        if size is not None:
            raise ValueError(f"size = (h, w) goes with pixel_format = {_YUV_LIST}; RGB frames carry their size in their shape")
        return None
    try:
        h, w = size
        ok = int(h) == h and int(w) == w
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"pixel_format = {pixel_format!r} needs size = (h, w), got {size!r}")
    if h < 2 or w < 2:
        raise ValueError(f"SAVSR needs h, w >= 2, got {h} x {w}")
    return int(h), int(w)


def check_colours(colour, out_colour, pixel_format: str, out: str) -> Tuple[int, int]:
    """The colour space ids (yuv.COLOURS) of the I420 input and output.  `colour` goes with pixel_format = 'i420' and `out_colour` with
    out = 'i420'; out_colour = None: the same as colour."""
    cid = check_colour(colour, "colour")
    ocid = cid if out_colour is None else check_colour(out_colour, "out_colour")
    if cid != 0 and pixel_format not in YUV_FORMATS:
        raise ValueError(f"colour = {colour!r} goes with pixel_format = {_YUV_LIST}: it is the colour space of YUV input (RGB frames have none)")
    if out_colour is not None and out not in YUV_FORMATS:
        raise ValueError(f"out_colour = {out_colour!r} goes with out = {_YUV_LIST}: it is the colour space of YUV output")
    return cid, ocid


def check_depths(depth, out_depth, pixel_format: str, out: str, colour: str = "bt601", out_colour: Optional[str] = None) -> Tuple[int, int]:
    """The bit depths (8, 10 or 12) of the I420 input and output.  `depth` goes with pixel_format = 'i420' and `out_depth` with
    out = 'i420'; out_depth = None: the same as depth (8 for RGB input).  10 and 12 bits are defined for the limited-range colour
    spaces only."""
    d = check_depth(depth, "depth")
    od = None if out_depth is None else check_depth(out_depth, "out_depth")
    if d != 8 and pixel_format not in SAMPLE_FORMATS:
        raise ValueError(f"depth = {d} goes with pixel_format = {_YUV_LIST}: it is the bit depth of YUV input (RGB frames carry theirs in their dtype)")
    if od is not None and out not in SAMPLE_FORMATS:
        raise ValueError(f"out_depth = {od} goes with out = {_YUV_LIST}: it is the bit depth of YUV output")
    if od is None:
        od = d if out in SAMPLE_FORMATS else 8
    check_depth_colour(d, colour, "depth", "colour")
    if out in SAMPLE_FORMATS:
        check_depth_colour(od, colour if out_colour is None else out_colour, "out_depth", "out_colour")
    return d, od


def check_sitings(siting, out_siting, pixel_format: str, out: str) -> Tuple[int, int]:
    """The chroma siting ids (0 = None: not modelled; else the position in yuv.SITINGS plus one) of the YUV input and output.  `siting`
    goes with a YUV pixel_format and `out_siting` with a YUV out; the two are independent (out_siting = None is not "the same")."""
    sid = check_siting(siting, chroma_of(pixel_format), "siting")
    osid = check_siting(out_siting, chroma_of(out), "out_siting")
    if siting is not None and pixel_format not in YUV_FORMATS:
        raise ValueError(f"siting = {siting!r} goes with pixel_format = {_YUV_LIST}: it is the chroma siting of YUV input (RGB frames have no chroma planes)")
    if out_siting is not None and out not in YUV_FORMATS:
        raise ValueError(f"out_siting = {out_siting!r} goes with out = {_YUV_LIST}: it is the chroma siting of YUV output")
    return sid, osid


def check_sample_alignment(frames: torch.Tensor, depth: int, chroma: str = "420") -> None:
    """10- and 12-bit frames are read as 16-bit words: their base pointer must be 2-byte aligned (a frame's byte size is always even)."""
    if depth > 8 and frames.numel() and frames.data_ptr() % 2:
        raise ValueError(f"{depth}-bit {layout_name(chroma)} frames hold 16-bit samples: the base pointer {frames.data_ptr():#x} is not 2-byte aligned "
                         f"(an odd storage offset of a uint8 view); copy the frames (.clone()) first")


def i420_layout(frames: torch.Tensor, size: Tuple[int, int], nch: int, depth: int = 8, chroma: str = "420", luma: bool = False) -> int:
    """N of a YUV video tensor: [N, frame_bytes(h, w, depth, chroma)] uint8 (GPU or host); refuses anything else, naming the layout and
    the byte count it expects.  luma: the luma-only path (`luma_mode`), where the network takes num_in_ch = 1 and chroma may be yuv.MONO."""
    h, w = size
    name, fb = layout_name(chroma), frame_bytes(h, w, depth, chroma)
    if not isinstance(frames, torch.Tensor):
        raise TypeError(f"frames must be a torch.Tensor, got {type(frames).__name__}")
    if nch != 3 and not (luma and nch == 1):
        raise ValueError(f"{name} frames are colour frames, the network takes num_in_ch = {nch}")
    if frames.dtype != torch.uint8:
        raise ValueError(f"{name} frames must be uint8, got {frames.dtype}")
    if frames.dim() != 2:
        raise ValueError(f"{name} frames must be [N, {'i420_bytes(h, w)' if chroma == '420' else 'frame_bytes(h, w, depth, chroma)'}] uint8, "
                         f"got {frames.dim()} dimensions")
    if depth != 8:
        if int(frames.shape[1]) != fb:
            raise ValueError(f"{depth}-bit {name} frames of {h} x {w} have {fb} bytes (16-bit samples), got {int(frames.shape[1])}")
        check_sample_alignment(frames, depth, chroma)
    elif int(frames.shape[1]) != fb:
        raise ValueError(f"{name} frames of {h} x {w} have {fb} bytes, got {int(frames.shape[1])}")
    return int(frames.shape[0])


def check_out(out: str, nch: int, chroma_filter: Optional[str] = None) -> None:
    if out not in OUT_KINDS and out != LUMA_FORMAT:
        raise ValueError(f"out = {out!r}: one of {', '.join(OUT_KINDS)}")
    if out in YUV_FORMATS and nch != 3 and not (nch == 1 and chroma_filter is not None):
        raise ValueError(f"out = {out!r} holds colour frames, the network gives num_in_ch = {nch}"
                         f"{' (a luma-only network writes them with chroma_filter = ' + repr('bicubic') + ')' if nch == 1 else ''}")


def luma_mode(nch: int, chroma_filter: Optional[str], pixel_format: str, out: str, colour: str, out_colour: Optional[str]) -> bool:
    """Whether the call takes the luma-only path: a num_in_ch = 1 network with chroma_filter or grey-scale ("y400") frames on either side.
    Refuses, by name, what that path cannot do.  False: the call runs the lines it ran before chroma_filter existed."""
    check_chroma_filter(chroma_filter)
    if chroma_filter is not None and nch != 1:
        raise ValueError(f"chroma_filter = {chroma_filter!r} with num_in_ch = {nch}: chroma goes through such a network; the filter is for "
                         f"luma-only networks (num_in_ch = 1)")
    for what, fmt in (("pixel_format", pixel_format), ("out", out)):
        if fmt == LUMA_FORMAT and nch != 1:
            raise ValueError(f"{what} = {fmt!r} holds grey-scale frames, the network takes num_in_ch = {nch}")
    if nch != 1 or not (chroma_filter is not None or LUMA_FORMAT in (pixel_format, out)):
        return False
    if pixel_format not in SAMPLE_FORMATS:
        if out in SAMPLE_FORMATS:
            raise ValueError(f"out = {out!r} from a luma-only network goes with pixel_format = {_YUV_LIST} or {LUMA_FORMAT!r}: RGB-layout frames "
                             f"have no planes to take the chroma from")
        raise ValueError(f"chroma_filter = {chroma_filter!r} goes with pixel_format = {_YUV_LIST}: {pixel_format!r} frames have no chroma planes "
                         f"to resample")
    if pixel_format == LUMA_FORMAT and out in YUV_FORMATS:
        raise ValueError(f"pixel_format = {LUMA_FORMAT!r} frames have no chroma planes: out = {out!r} cannot be made from them")
    if out_colour is not None and out_colour != colour:
        raise ValueError(f"colour = {colour!r}, out_colour = {out_colour!r}: a luma-only network never forms RGB, so the samples keep their "
                         f"colour space")
    return True


@dataclass(frozen=True)
class Side:
    """The frames on one side of the network, by name: the pixel format / output kind ("rgb", "float", "uint8", "i420", "i422", "i444",
    "y400"), the layout of its planes ("420", "422", "444", yuv.MONO; None for packed frames), the bit depth, the colour space and the
    chroma siting (None: not modelled).  A record without checks of its own: `video_spec` is what makes a checked pair of them."""
    fmt: str
    layout: Optional[str]
    depth: int
    colour: str
    siting: Optional[str]

    @property
    def yuv(self) -> bool:
        """Planar YUV frames (i420, i422, i444): the side has chroma planes, a colour space and a siting."""
        return self.fmt in YUV_FORMATS

    @property
    def planar(self) -> bool:
        """Frames of planar samples with a bit depth, [N, frame_bytes] uint8: YUV or grey-scale."""
        return self.fmt in SAMPLE_FORMATS

    def frame_bytes(self, h: int, w: int) -> int:
        return frame_bytes(h, w, self.depth, self.layout)


def check_dither_out(dither, out: str) -> Optional[str]:
    """`dither` (None or one of dither.DITHERS) goes with an integer output: out = 'float' has nothing to quantise."""
    check_dither(dither)
    if dither is not None and out == "float":
        raise ValueError(f"dither = {dither!r} goes with an integer output (out = 'uint8', {_YUV_LIST} or {LUMA_FORMAT!r}): out = 'float' has "
                         f"nothing to quantise")
    return dither


def _resolve(nch: int, out: str, pixel_format: str, size, colour, out_colour, depth, out_depth, siting, out_siting, chroma_filter, dither=None):
    """The fields of the VideoSpec of these arguments, after every check of them, in the order and the words the checks always had."""
    check_out(out, nch, chroma_filter)
    size = check_pixel_format(pixel_format, size)
    check_colours(colour, out_colour, pixel_format, out)
    d, od = check_depths(depth, out_depth, pixel_format, out, colour, out_colour)
    check_sitings(siting, out_siting, pixel_format, out)
    luma = luma_mode(nch, chroma_filter, pixel_format, out, colour, out_colour)
    check_dither_out(dither, out)
    return (nch, Side(pixel_format, layout_of(pixel_format) if size else None, d, colour, siting),
            Side(out, layout_of(out) if out in SAMPLE_FORMATS else None, od, colour if out_colour is None else out_colour, out_siting),
            size, luma, chroma_filter, dither)


@dataclass(frozen=True)
class VideoSpec:
    """Everything about the frames of a video call, on both sides of the network, checked: what `upscale_video`, `VideoUpscaler`, the
    cut detector and `HipEngine.forward_video` read.  Names only; the ids of the C ABI are computed next to the calls that take them.
    Built by `video_spec`; building one any other way runs the same checks on its fields, so there is no invalid VideoSpec."""
    nch: int                                  # the network's num_in_ch: the channels of packed frames
    inp: Side
    out: Side
    size: Optional[Tuple[int, int]]           # (h, w) of planar input frames; None: packed ones, which carry it in their shape
    luma: bool                                # the luma-only path (`luma_mode`)
    chroma_filter: Optional[str]
    dither: Optional[str] = None              # the quantiser's dither (dither.DITHERS); None: round to nearest

    def __post_init__(self):
        fields = (self.nch, self.inp, self.out, self.size, self.luma, self.chroma_filter, self.dither)
        if not isinstance(self.inp, Side) or not isinstance(self.out, Side) or _resolve(
                self.nch, self.out.fmt, self.inp.fmt, self.size, self.inp.colour, self.out.colour if self.out.yuv else None, self.inp.depth,
                self.out.depth if self.out.planar else None, self.inp.siting, self.out.siting, self.chroma_filter, self.dither) != fields:
            raise ValueError(f"not the VideoSpec of its own arguments (video_spec builds one): {fields}")

    @property
    def out_kind(self) -> str:
        """What the engine returns: "float" [n, c, H, W], "uint8" [n, H, W, c] or "planar" [n, out.frame_bytes(H, W)] uint8."""
        return "planar" if self.out.planar else self.out.fmt

    def frames_hw(self, frames: torch.Tensor) -> Tuple[int, int, int]:
        """(N, h, w) of a video tensor of the input side (`i420_layout` / `frame_layout`: refuses anything else)."""
        if self.size:
            return (i420_layout(frames, self.size, self.nch, self.inp.depth, self.inp.layout, self.luma),) + self.size
        return frame_layout(frames, self.nch)


def video_spec(nch: int, out: str = "float", pixel_format: str = "rgb", size=None, colour: str = "bt601", out_colour: Optional[str] = None,
               depth: int = 8, out_depth: Optional[int] = None, siting: Optional[str] = None, out_siting: Optional[str] = None,
               chroma_filter: Optional[str] = None, dither: Optional[str] = None) -> VideoSpec:
    """The VideoSpec of the format arguments of `upscale_video` / `VideoUpscaler` for a num_in_ch = nch network; refuses, by name, what
    they refuse.  dither: None or one of dither.DITHERS, the rule of every quantiser behind the network (savsr_amd/dither.py)."""
    return VideoSpec(*_resolve(nch, out, pixel_format, size, colour, out_colour, depth, out_depth, siting, out_siting, chroma_filter, dither))


def detector_layout(frames: torch.Tensor, side: Side, size: Optional[Tuple[int, int]]) -> Tuple[int, int, int, int]:
    """(N, c, h, w) of the frames the stages in front of the network take (c = 0: planar ones, `size` = their (h, w)); no network here, so
    any c in 1 .. 3 and any h, w >= 1."""
    depth, chroma = side.depth, side.layout
    if not isinstance(frames, torch.Tensor):
        raise TypeError(f"frames must be a torch.Tensor, got {type(frames).__name__}")
    if depth != 8 and not size:
        raise ValueError(f"depth = {depth} goes with pixel_format = {_YUV_LIST}: it is the bit depth of YUV input (RGB frames carry theirs in their dtype)")
    if size:
        h, w = size
        if frames.dtype != torch.uint8 or frames.dim() != 2 or int(frames.shape[1]) != side.frame_bytes(h, w):
            raise ValueError(f"{'' if depth == 8 else f'{depth}-bit '}{layout_name(chroma)} frames of {h} x {w} are "
                             f"[N, {side.frame_bytes(h, w)}] uint8, got {frames.dtype} {tuple(frames.shape)}")
        check_sample_alignment(frames, depth, chroma)
        n, c = int(frames.shape[0]), 0
    else:
        n, c, h, w = _packed_dims(frames)
        if not 1 <= c <= 3:
            raise ValueError(f"frames have {c} channels: 1 .. 3")
        if h < 1 or w < 1:
            raise ValueError(f"frames of {h} x {w}")
    if n < 1:
        raise ValueError("the video has no frames")
    return n, c, h, w


def detector_side(pixel_format: str, size, depth) -> Tuple[Side, Optional[Tuple[int, int]]]:
    """The input side and the frame size the public stage calls name (pair_sad, line_sums, deinterlace, ...: they read no colour space and
    no siting)."""
    size = check_pixel_format(pixel_format, size)
    return Side(pixel_format, layout_of(pixel_format) if size else None, check_depth(depth), "bt601", None), size


# ---- the plane table: where the byte matrices of a frame lie ---------------------------------------------------------------------------
_BLOCK = {"420": (2, 2), "422": (1, 2), "444": (1, 1), MONO: (1, 1), None: (1, 1)}          # (vertical, horizontal) chroma block of a layout


def block_of(layout: Optional[str]) -> Tuple[int, int]:
    """(vertical, horizontal) luma samples per chroma sample of a layout; (1, 1) for "444", grey-scale ("400") and packed frames (None)."""
    if layout not in _BLOCK:
        raise ValueError(f"layout = {layout!r}: one of 420, 422, 444, {MONO} or None (packed frames)")
    return _BLOCK[layout]


class Plane(NamedTuple):
    """One byte matrix of a frame, `offset` bytes into it; a sample stands for bv x bh luma samples (the chroma block; else (1, 1))."""
    offset: int
    rows: int
    row_bytes: int
    bv: int
    bh: int


class PlaneTable(NamedTuple):
    """A frame's byte stride, its sample size in bytes (2 at depth 10 / 12) and its byte matrices in order: entry 0 is "the Y matrix" (the
    whole frame for packed ones), a loop over them is "every plane"."""
    stride: int
    sample: int
    planes: Tuple[Plane, ...]


def plane_table(side: Side, size: Optional[Tuple[int, int]], c: int = 0, h: int = 0, w: int = 0) -> PlaneTable:
    """The PlaneTable of a frame kind.  Planar frames (`size` = their (h, w); c, h, w are not read): Y, then U and V unless the side is
    grey-scale, contiguous, ending at side.frame_bytes(h, w).  Packed uint8 frames (size = None) of h x w pixels of c bytes: one
    h x (w * c) matrix.  fp32 CHW frames have no byte matrices: the two stages that accept them branch before they ask."""
    if not size:
        return PlaneTable(h * w * c, 1, (Plane(0, h, w * c, 1, 1),))
    h, w = size
    s = 1 if side.depth == 8 else 2
    planes = [Plane(0, h, w * s, 1, 1)]
    if side.layout != MONO:
        ch, cw = chroma_hw(h, w, side.layout)
        bv, bh = block_of(side.layout)
        planes += [Plane(h * w * s, ch, cw * s, bv, bh), Plane((h * w + ch * cw) * s, ch, cw * s, bv, bh)]
    return PlaneTable(side.frame_bytes(h, w), s, tuple(planes))
