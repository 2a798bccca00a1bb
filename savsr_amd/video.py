"""Whole LR videos in, SR videos out: the sequence path behind `SAVSR.upscale_video` and `VideoUpscaler`.

Output frame i is what the reference pipeline gives for it: the frame's window by generate_frame_indices with the chosen padding
(lbasicsr/data/data_util.py:63-112, `harness.window_indices`), then SAVSR.forward on that window; with out="uint8", tensor2img's
clamp / x255 / round half to even (lbasicsr/utils/img_util.py:66-90) without the BGR swap.  The frames stay on the device: the
windows are gathered there and the result is quantised there, by one path for every kind of frame, HipEngine.forward_video.

What the frames on either side of the network are -- pixel_format / out, size, depth / out_depth, colour / out_colour, siting /
out_siting, chroma_filter and the network's num_in_ch -- is one value, a `VideoSpec`: `video_spec` checks the arguments, once, in a fixed
order, and everything behind it (upscale_video, VideoUpscaler, the cut detector, the engine) reads the spec and checks nothing again.  It
holds names only; the integer ids of the C ABI are computed beside the calls that take them.
pixel_format="i420" / out="i420": planar YUV 4:2:0 frames in / out (savsr_amd/yuv.py is the format and its numerics), converted on the
device on either side of the network.  depth / out_depth = 10, 12: the frames hold little-endian 16-bit samples
([N, 2 * i420_bytes(h, w)] uint8, Y4M's C420p10 / C420p12), limited range only.  pixel_format / out = "i422", "i444": the 4:2:2 and 4:4:4
layouts of the same planes ([N, yuv.frame_bytes(h, w, depth, chroma)] uint8), with everything above applying to them as well; the two
sides are independent.  siting / out_siting: the chroma siting of the YUV input / output (yuv.SITINGS; linear chroma reconstruction in,
cosited filters out; None = not modelled: nearest up, box down).  Every YUV side goes through one entry, savsr_video_gather_yuvs /
savsr_video_quantize_yuvs.

cuts=[k, ...] / cuts="auto": the video is a sequence of scenes and every scene is treated as a video of its own (savsr_amd/scenes.py:
windows stop at cuts); "auto" finds the cuts on the device (savsr_video_pair_sad_*, then scdet's rule on the host).  cuts=None runs
exactly the lines it ran before cuts existed.

chroma_filter="bicubic" with a num_in_ch = 1 network (a luma-only checkpoint): YUV frames in and out are accepted; the Y plane goes
through the network (savsr_video_gather_luma / savsr_video_quantize_luma) and every output frame's U and V are resampled from its own
input frame at the network's scale (savsr_video_resample_chroma; savsr_amd/yuv.py "Luma-only checkpoints" is the specification).
pixel_format / out = "y400": grey-scale frames, the Y plane alone (Y4M's Cmono), for such a network; it needs no chroma_filter.
chroma_filter=None refuses what it refused before the argument existed.

crop=(y0, x0, ah, aw) / crop="auto": letterboxed video.  The frames are cropped to the rect before anything else looks at them, so the
call is, bit for bit, the call on the hand-cropped video (savsr_amd/active.py); "auto" finds the rect on the device
(savsr_video_line_sums_*, then cropdetect's rule on the host).  bars="keep" puts the result back into full-size frames of nominal black,
bars="drop" returns the picture alone.  The crop and the re-insertion are strided copies through torch views.  crop=None runs exactly
the lines it ran before.

fields="tff" / "bff": interlaced video.  The N frames become 2N progressive frames at the field rate before anything else looks at
them -- before the crop -- so the call is, bit for bit, the call on `deinterlace(frames, fields, ...)` (savsr_amd/deinterlace.py is the
specification: ffmpeg yadif's rule in integers; savsr_video_deinterlace_u8 / _u16 once per plane).  fields=None runs exactly the lines it
ran before.

pulldown="tff" / "bff": telecined film (3:2 pulldown).  The N frames become the N - N // pulldown_cycle film frames before anything else
looks at them -- where fields= comes, which it excludes -- so the call is, bit for bit, the call on `remove_pulldown(frames, pulldown, ...)`
(savsr_amd/pulldown.py is the specification: savsr_video_field_scores_* and a host decision match the fields, savsr_video_weave puts them
together, savsr_video_pair_sad_* and a host decision drop the repeated frame of every cycle).  pulldown=None runs exactly the lines it
ran before.

Every argument is checked here, on the host, before anything is enqueued on the GPU.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import torch

from .harness import window_indices
from .yuv import (CHROMA_OF, CHROMAS, LUMA_FORMAT, MONO, check_chroma_filter, check_colour, check_depth, check_depth_colour, check_siting, frame_bytes,
                  i420_bytes, layout_name)

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


def frame_layout(frames: torch.Tensor, nch: int) -> Tuple[int, int, int]:
    """(N, h, w) of a video tensor: [N, h, w, c] uint8 (GPU or host) or [N, c, h, w] float on the GPU; refuses anything else."""
    if not isinstance(frames, torch.Tensor):
        raise TypeError(f"frames must be a torch.Tensor, got {type(frames).__name__}")
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
    if c != nch:
        raise ValueError(f"frames have {c} channels, the network takes num_in_ch = {nch}")
    if h < 2 or w < 2:
        raise ValueError(f"SAVSR needs h, w >= 2, got {h} x {w}")
    return int(n), int(h), int(w)


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


def _to_device(frames: torch.Tensor, device: torch.device) -> torch.Tensor:
    if frames.device == device:
        return frames
    if frames.is_cuda:
        raise RuntimeError(f"frames on {frames.device}, network on {device}")
    from ._xfer import h2d
    return h2d(frames.contiguous(), device)


def _check_net(net) -> None:
    if net.training:
        raise RuntimeError("savsr_amd.SAVSR implements the inference path only; call .eval() first")


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


def _resolve(nch: int, out: str, pixel_format: str, size, colour, out_colour, depth, out_depth, siting, out_siting, chroma_filter):
    """The fields of the VideoSpec of these arguments, after every check of them, in the order and the words the checks always had."""
    check_out(out, nch, chroma_filter)
    size = check_pixel_format(pixel_format, size)
    check_colours(colour, out_colour, pixel_format, out)
    d, od = check_depths(depth, out_depth, pixel_format, out, colour, out_colour)
    check_sitings(siting, out_siting, pixel_format, out)
    luma = luma_mode(nch, chroma_filter, pixel_format, out, colour, out_colour)
    return (nch, Side(pixel_format, layout_of(pixel_format) if size else None, d, colour, siting),
            Side(out, layout_of(out) if out in SAMPLE_FORMATS else None, od, colour if out_colour is None else out_colour, out_siting),
            size, luma, chroma_filter)


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

    def __post_init__(self):
        fields = (self.nch, self.inp, self.out, self.size, self.luma, self.chroma_filter)
        if not isinstance(self.inp, Side) or not isinstance(self.out, Side) or _resolve(
                self.nch, self.out.fmt, self.inp.fmt, self.size, self.inp.colour, self.out.colour if self.out.yuv else None, self.inp.depth,
                self.out.depth if self.out.planar else None, self.inp.siting, self.out.siting, self.chroma_filter) != fields:
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
               chroma_filter: Optional[str] = None) -> VideoSpec:
    """The VideoSpec of the format arguments of `upscale_video` / `VideoUpscaler` for a num_in_ch = nch network; refuses, by name, what
    they refuse."""
    return VideoSpec(*_resolve(nch, out, pixel_format, size, colour, out_colour, depth, out_depth, siting, out_siting, chroma_filter))


def _is_auto(cuts) -> bool:
    return isinstance(cuts, str) and cuts == "auto"


def check_cuts_arg(cuts) -> None:
    """cuts is None, "auto" or a sequence of frame indices (the indices themselves: scenes.check_cuts, once the length is known)."""
    if cuts is None or _is_auto(cuts):
        return
    if isinstance(cuts, (str, bytes)):
        raise ValueError(f"cuts = {cuts!r}: None, 'auto' or a sequence of frame indices")
    from .scenes import check_cuts
    check_cuts(cuts, None)


def _sad_layout(frames: torch.Tensor, side: Side, size: Optional[Tuple[int, int]]) -> Tuple[int, int, int, int]:
    """(N, c, h, w) of the frames the detector compares (c = 0: planar ones, `size` = their (h, w)); no network here, so any c in 1 .. 3
    and any h, w >= 1."""
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
        if frames.dim() != 4:
            raise ValueError(f"frames must be [N, h, w, c] uint8 or [N, c, h, w] float, got {frames.dim()} dimensions")
        if frames.dtype == torch.uint8:
            n, h, w, c = (int(v) for v in frames.shape)
        elif frames.is_floating_point():
            if not frames.is_cuda:
                raise ValueError("float frames must be on the GPU ([N, c, h, w]); host frames go as [N, h, w, c] uint8")
            n, c, h, w = (int(v) for v in frames.shape)
        else:
            raise ValueError(f"frames must be uint8 or float, got {frames.dtype}")
        if not 1 <= c <= 3:
            raise ValueError(f"frames have {c} channels: 1 .. 3")
        if h < 1 or w < 1:
            raise ValueError(f"frames of {h} x {w}")
    if n < 1:
        raise ValueError("the video has no frames")
    return n, c, h, w


def _pair_sad_device(frames: torch.Tensor, side: Side, size: Optional[Tuple[int, int]]) -> torch.Tensor:
    """savsr_video_pair_sad_* on frames of the input side already on the GPU: int64 [N - 1] there, enqueued on the current stream (no sync)."""
    from . import _lib
    n, c, h, w = _sad_layout(frames, side, size)
    depth, chroma = side.depth, side.layout
    lib = _lib.load()
    u8 = frames.dtype == torch.uint8
    frames = frames.contiguous() if u8 else frames.to(torch.float32).contiguous()
    with torch.cuda.device(frames.device):
        sad = torch.empty(n - 1, dtype=torch.int64, device=frames.device)
        st = torch.cuda.current_stream().cuda_stream
        if size and chroma == MONO:
            # grey-scale frames are [N, h, w, 1] frames of their samples' 8 most significant bits (host work only: no kernel of their own)
            if depth != 8:
                words = frames.view(torch.int16).to(torch.int32) & 0xFFFF
                frames = (words.clamp_(max=(1 << depth) - 1) >> (depth - 8)).to(torch.uint8)
            _lib.check(lib.savsr_video_pair_sad_u8(frames.data_ptr(), n, 1, h, w, sad.data_ptr(), st), "savsr_video_pair_sad_u8")
        elif size and chroma != "420":
            _lib.check(lib.savsr_video_pair_sad_yuvp(frames.data_ptr(), n, h, w, depth, CHROMAS.index(chroma), sad.data_ptr(), st),
                       "savsr_video_pair_sad_yuvp")
        elif size and depth != 8:
            _lib.check(lib.savsr_video_pair_sad_i420_16(frames.data_ptr(), n, h, w, depth, sad.data_ptr(), st), "savsr_video_pair_sad_i420_16")
        elif size:
            _lib.check(lib.savsr_video_pair_sad_i420(frames.data_ptr(), n, h, w, sad.data_ptr(), st), "savsr_video_pair_sad_i420")
        elif u8:
            _lib.check(lib.savsr_video_pair_sad_u8(frames.data_ptr(), n, c, h, w, sad.data_ptr(), st), "savsr_video_pair_sad_u8")
        else:
            _lib.check(lib.savsr_video_pair_sad_f32(frames.data_ptr(), n, c, h, w, sad.data_ptr(), st), "savsr_video_pair_sad_f32")
    return sad


def _sad_side(pixel_format: str, size, depth) -> Tuple[Side, Optional[Tuple[int, int]]]:
    """The input side and the frame size the public detector calls name (the detector reads no colour space and no siting)."""
    size = check_pixel_format(pixel_format, size)
    return Side(pixel_format, layout_of(pixel_format) if size else None, check_depth(depth), "bt601", None), size


def _sad_device(frames: torch.Tensor) -> torch.device:
    if frames.is_cuda:
        return frames.device
    if not torch.cuda.is_available():
        raise RuntimeError("savsr_amd runs on an AMD GPU only: the detector's scores are computed there")
    return torch.device("cuda", torch.cuda.current_device())


def pair_sad(frames: torch.Tensor, pixel_format: str = "rgb", size=None, depth: int = 8) -> torch.Tensor:
    """The scene detector's scores: int64 [N - 1] on the GPU, entry j = the sum of absolute differences of the 8-bit samples of frames j
    and j + 1 (savsr_amd.scenes.pair_sad is the specification).  frames as for SAVSR.upscale_video, with any c in 1 .. 3: [N, h, w, c]
    uint8 (GPU or host; every byte), [N, c, h, w] float on the GPU (every value after the uint8 output's quantisation), or with
    pixel_format="i420", size=(h, w): [N, i420_bytes(h, w)] uint8 (the Y plane only).  depth = 10, 12 (I420 only): frames of 16-bit samples,
    [N, 2 * i420_bytes(h, w)] uint8, compared by their 8 most significant bits, so the scores keep the 8-bit scale.  pixel_format="i422" /
    "i444": frames of those layouts; the Y plane only, as for I420."""
    side, size = _sad_side(pixel_format, size, depth)
    _sad_layout(frames, side, size)
    return _pair_sad_device(_to_device(frames, _sad_device(frames)), side, size)


def detect_cuts(frames: torch.Tensor, threshold=10.0, pixel_format: str = "rgb", size=None, depth: int = 8) -> List[int]:
    """The scene cuts of a video: the frames k whose change from frame k - 1, damped by the previous pair's, is at least `threshold`
    per cent of the largest possible one (ffmpeg scdet's rule in exact integer arithmetic, savsr_amd.scenes.cuts_from_sad, on pair_sad's
    scores; one device -> host copy of N - 1 integers).  The default threshold is scdet's and is not validated on real footage."""
    from .scenes import check_threshold, cuts_from_sad, sad_samples
    check_threshold(threshold)
    _sad_layout(frames, *_sad_side(pixel_format, size, depth))
    sad = pair_sad(frames, pixel_format, size, depth)
    return cuts_from_sad(sad.cpu().tolist(), sad_samples(frames.shape, pixel_format, size), threshold)


# ---- the active picture (savsr_amd/active.py is the specification) ----------------------------------------------------------------------
def _line_sums_device(frames: torch.Tensor, side: Side, size: Optional[Tuple[int, int]]) -> Tuple[torch.Tensor, torch.Tensor]:
    """savsr_video_line_sums_* on frames of the input side already on the GPU: int64 ([N, h], [N, w]) there, enqueued on the current stream
    (no sync).  Every frame kind is host work over the three entries: which matrix, which stride, and the folding of their sums."""
    from . import _lib
    n, c, h, w = _sad_layout(frames, side, size)
    depth = side.depth
    lib = _lib.load()
    u8 = frames.dtype == torch.uint8
    frames = frames.contiguous() if u8 else frames.to(torch.float32).contiguous()
    with torch.cuda.device(frames.device):
        st = torch.cuda.current_stream().cuda_stream
        mats, width = (n, w) if size else ((n, w * c) if u8 else (n * c, w))
        cells = torch.empty(mats * (h + width), dtype=torch.int32, device=frames.device)          # (one buffer: the entry zeroes it in one memset)
        rows, cols = cells[:mats * h].view(mats, h), cells[mats * h:].view(mats, width)
        if size and depth != 8:
            _lib.check(lib.savsr_video_line_sums_u16(frames.data_ptr(), n, side.frame_bytes(h, w), h, w, depth, rows.data_ptr(), cols.data_ptr(), st),
                       "savsr_video_line_sums_u16")
        elif size:
            _lib.check(lib.savsr_video_line_sums_u8(frames.data_ptr(), n, side.frame_bytes(h, w), h, w, rows.data_ptr(), cols.data_ptr(), st),
                       "savsr_video_line_sums_u8")
        elif u8:
            _lib.check(lib.savsr_video_line_sums_u8(frames.data_ptr(), n, h * w * c, h, w * c, rows.data_ptr(), cols.data_ptr(), st),
                       "savsr_video_line_sums_u8")
            cols = cols.view(n, w, c)          # (a cell is below 2^32: as int64 before the channels are folded)
        else:
            _lib.check(lib.savsr_video_line_sums_f32(frames.data_ptr(), n * c, h, w, rows.data_ptr(), cols.data_ptr(), st), "savsr_video_line_sums_f32")
            rows, cols = rows.view(n, c, h), cols.view(n, c, w)
        rows, cols = (t.to(torch.int64) & 0xFFFFFFFF for t in (rows, cols))          # the cells are unsigned
        if not size and u8:
            cols = cols.sum(2)
        elif not size:
            rows, cols = rows.sum(1), cols.sum(1)
    return rows, cols


def line_sums(frames: torch.Tensor, pixel_format: str = "rgb", size=None, depth: int = 8) -> Tuple[torch.Tensor, torch.Tensor]:
    """The active-picture detector's line sums: int64 ([N, h], [N, w]) on the GPU, per frame the sum of the 8-bit samples of every row
    and of every column (savsr_amd.active.line_sums is the specification), on the caller's current stream, without a sync.  frames as for
    `pair_sad`, and the same samples: every byte of [N, h, w, c] uint8 frames (GPU or host), every value of [N, c, h, w] float frames on the
    GPU after the uint8 output's quantisation, the Y plane of planar frames (pixel_format=, size=(h, w); at depth 10 / 12 a sample's 8
    most significant bits)."""
    side, size = _sad_side(pixel_format, size, depth)
    _sad_layout(frames, side, size)
    return _line_sums_device(_to_device(frames, _sad_device(frames)), side, size)


def _detect_device(frames: torch.Tensor, side: Side, size: Optional[Tuple[int, int]], limit) -> Tuple[int, int, int, int]:
    """The aligned active rect of frames of the input side on the GPU: the line sums, their maxima over the frames on the device, one
    device -> host copy of h + w integers, then active_rect and align_rect on the host."""
    from . import active
    n, c, h, w = _sad_layout(frames, side, size)
    rows, cols = _line_sums_device(frames, side, size)
    top = torch.cat([rows.amax(0), cols.amax(0)]).cpu().tolist()
    s_row, s_col = active.line_samples(h, w, max(c, 1))
    return active.align_rect(active.active_rect(top[:h], top[h:], s_row, s_col, limit), side.layout)


def detect_active_area(frames: torch.Tensor, limit=24, pixel_format: str = "rgb", size=None, depth: int = 8) -> Tuple[int, int, int, int]:
    """The active picture (y0, x0, ah, aw) of a letterboxed, pillarboxed or window-boxed video: ffmpeg cropdetect's rule in exact integer
    arithmetic (savsr_amd.active.active_rect) on `line_sums`: a row or column whose mean sample stays at or below `limit` (the 8-bit
    scale) in every frame is bar, the picture spans the first to the last line that is not; the offsets are then moved outwards to the
    chroma block of the layout (active.align_rect).  No picture, or one below 2 x 2: the whole frame.  The default limit is cropdetect's
    and is not validated on real footage."""
    from . import active
    active.check_limit(limit)
    side, size = _sad_side(pixel_format, size, depth)
    _sad_layout(frames, side, size)
    return _detect_device(_to_device(frames, _sad_device(frames)), side, size, limit)


def _plane_table(h: int, w: int, side: Side):
    """[(byte offset, rows, row bytes, vertical block, horizontal block)] of the planes of a planar h x w frame of `side`."""
    from .active import block_of
    from .yuv import chroma_hw
    s = 1 if side.depth == 8 else 2
    table = [(0, h, w * s, 1, 1)]
    if side.layout != MONO:
        ch, cw = chroma_hw(h, w, side.layout)
        bv, bh = block_of(side.layout)
        table += [(h * w * s, ch, cw * s, bv, bh), ((h * w + ch * cw) * s, ch, cw * s, bv, bh)]
    return table


def _crop_device(frames: torch.Tensor, rect, side: Side, hw: Tuple[int, int]) -> torch.Tensor:
    """active.crop_frames on a device tensor: strided copies through views.  Planar frames: every plane sliced at the rect divided by its
    block and the slices concatenated (bytes; a 16-bit sample is two of them, so the offsets stay even)."""
    y0, x0, ah, aw = rect
    if not side.planar:
        if frames.dtype == torch.uint8:
            return frames[:, y0:y0 + ah, x0:x0 + aw].contiguous()
        return frames[:, :, y0:y0 + ah, x0:x0 + aw].contiguous()
    h, w = hw
    n, s = frames.shape[0], 1 if side.depth == 8 else 2
    parts = []
    for (off, ph, pb, _, _), (_, qh, qb, bv, bh) in zip(_plane_table(h, w, side), _plane_table(ah, aw, side)):
        py, px = y0 // bv, (x0 // bh) * s
        parts.append(frames[:, off:off + ph * pb].view(n, ph, pb)[:, py:py + qh, px:px + qb].reshape(n, qh * qb))
    return torch.cat(parts, 1)


def _insert_device(sr: torch.Tensor, placed, spec: "VideoSpec") -> torch.Tensor:
    """active.insert_frames on a device tensor: full-size frames of active.bars_frame with the picture's planes copied in at (Y0, X0)
    divided by each plane's block."""
    from .active import bars_frame
    Hf, Wf, Ha, Wa, Y0, X0 = placed
    out, n = spec.out, sr.shape[0]
    bars = torch.from_numpy(bars_frame(Hf, Wf, out.fmt, out.depth, out.colour, spec.nch)).to(sr.device)
    full = bars.unsqueeze(0).repeat(n, *([1] * bars.dim()))
    if out.fmt == "float":
        full[:, :, Y0:Y0 + Ha, X0:X0 + Wa] = sr
    elif not out.planar:
        full[:, Y0:Y0 + Ha, X0:X0 + Wa] = sr
    else:
        s = 1 if out.depth == 8 else 2
        for (off, ph, pb, bv, bh), (aoff, qh, qb, _, _) in zip(_plane_table(Hf, Wf, out), _plane_table(Ha, Wa, out)):
            py, px = Y0 // bv, (X0 // bh) * s
            full[:, off:off + ph * pb].view(n, ph, pb)[:, py:py + qh, px:px + qb] = sr[:, aoff:aoff + qh * qb].view(n, qh, qb)
    return full


def _check_crop_args(crop, crop_limit, bars, auto_ok: bool = True):
    """crop is None, "auto" or a rect; bars / crop_limit go with a crop.  The rect itself: active.check_rect, once the frame size is known."""
    from . import active
    if crop is None:
        if bars != "keep":
            raise ValueError(f"bars = {bars!r} goes with crop=: without a crop there are no bars to keep or drop")
        if isinstance(crop_limit, bool) or crop_limit != active.DEFAULT_LIMIT:
            raise ValueError(f"crop_limit = {crop_limit!r} goes with crop=: it is the limit of the detector behind crop='auto'")
        return None
    active.check_bars(bars)
    active.check_limit(crop_limit)
    if isinstance(crop, str):
        if crop != "auto":
            raise ValueError(f"crop = {crop!r}: None, 'auto' or a rect (y0, x0, ah, aw) of ints")
        if not auto_ok:
            raise ValueError("crop = 'auto' in VideoUpscaler: the decision needs the whole video; detect the rect first "
                             "(savsr_amd.detect_active_area) and give it, or use python -m savsr_amd.upscale --crop auto")
        return crop
    return active.check_rect(crop, None, None, None)


def _cropped_spec(spec: "VideoSpec", rect) -> "VideoSpec":
    """The VideoSpec of the cropped frames: the same sides at the rect's size."""
    from dataclasses import replace
    return replace(spec, size=(rect[2], rect[3])) if spec.size else spec


# ---- interlaced video (savsr_amd/deinterlace.py is the specification) -----------------------------------------------------------------------
def _check_fields(fields) -> Optional[str]:
    if fields is None:
        return None
    from .deinterlace import check_order
    check_order(fields, "fields")
    return fields


def _field_frames(frames: torch.Tensor, side: Side, size: Optional[Tuple[int, int]]) -> Tuple[int, int, int, int]:
    """(N, c, h, w) of frames the deinterlacer takes (`_sad_layout`'s, N = 0 allowed); refuses float frames and frames whose matrices
    have one row."""
    from .deinterlace import check_frame_rows
    if isinstance(frames, torch.Tensor) and not size and frames.is_floating_point():
        raise ValueError("float frames have no integer samples to deinterlace: give [N, h, w, c] uint8 or planar frames (quantise first)")
    if isinstance(frames, torch.Tensor) and frames.dim() and int(frames.shape[0]) == 0:
        n, c, h, w = (0,) + _sad_layout(frames.new_zeros((1,) + tuple(frames.shape[1:])), side, size)[1:]
    else:
        n, c, h, w = _sad_layout(frames, side, size)
    check_frame_rows(h, side.layout)
    return n, c, h, w


def _deinterlace_device(frames: torch.Tensor, order: str, side: Side, size: Optional[Tuple[int, int]], lo: int = 0, hi: Optional[int] = None) -> torch.Tensor:
    """savsr_video_deinterlace_* on resident frames of the input side on the GPU: the 2 (hi - lo) progressive frames of source frames
    [lo, hi) (default: all), prev / next taken among the resident frames and clamped there.  One call per plane, on the current stream."""
    from . import _lib
    from .deinterlace import FIELD_ORDERS
    n, c, h, w = _field_frames(frames, side, size)
    hi = n if hi is None else hi
    frames = frames.contiguous()
    out = frames.new_empty((2 * (hi - lo),) + tuple(frames.shape[1:]))
    if hi <= lo:
        return out
    lib = _lib.load()
    oid = FIELD_ORDERS.index(order)
    with torch.cuda.device(frames.device):
        st = torch.cuda.current_stream().cuda_stream
        if not size:
            _lib.check(lib.savsr_video_deinterlace_u8(frames.data_ptr(), n, h * w * c, 0, h, w * c, c, oid, lo, hi, out.data_ptr(), h * w * c, 0, st),
                       "savsr_video_deinterlace_u8")
            return out
        fb = side.frame_bytes(h, w)
        for off, ph, pb, _, _ in _plane_table(h, w, side):
            if side.depth == 8:
                _lib.check(lib.savsr_video_deinterlace_u8(frames.data_ptr(), n, fb, off, ph, pb, 1, oid, lo, hi, out.data_ptr(), fb, off, st),
                           "savsr_video_deinterlace_u8")
            else:
                _lib.check(lib.savsr_video_deinterlace_u16(frames.data_ptr(), n, fb, off, ph, pb // 2, side.depth, oid, lo, hi, out.data_ptr(), fb, off, st),
                           "savsr_video_deinterlace_u16")
    return out


def deinterlace(frames: torch.Tensor, order: str, pixel_format: str = "rgb", size=None, depth: int = 8) -> torch.Tensor:
    """Interlaced video as progressive frames at the field rate: 2N frames on the GPU in the format of the N given ones
    (savsr_amd.deinterlace.deinterlace_frames is the specification, bit for bit), on the caller's current stream, without a sync.  Output
    frame 2n + f keeps field f of source frame n (order "tff": the top field is the earlier one; "bff": the bottom one) and interpolates
    the other rows by ffmpeg yadif's rule.  frames: [N, h, w, c] uint8 (GPU or host, c in 1 .. 3), or with pixel_format "i420", "i422",
    "i444", "y400" and size=(h, w): [N, frame_bytes] uint8, every plane on its own, 16-bit samples at depth 10 / 12.  Float frames are
    refused, and so are frames of one row (three for 4:2:0: the chroma planes need two)."""
    from .deinterlace import check_order
    check_order(order)
    side, size = _sad_side(pixel_format, size, depth)
    _field_frames(frames, side, size)
    return _deinterlace_device(_to_device(frames, _sad_device(frames)), order, side, size)


class FieldSplitter:
    """The streaming deinterlacer behind VideoUpscaler(fields=...): push(source frames on the GPU) returns the progressive frames that are
    final, finish() the last source frame's two.  The second field of the last pushed frame needs the frame after it, so one source frame
    is held back; with the frame before it (the temporal context) the device keeps at most two source frames between pushes (copies of
    their own, so that the chunk they came with is released).  Concatenated, the outputs are `deinterlace` on the whole video for any
    chunking.  finish() without a pushed frame returns None."""

    def __init__(self, order: str, side: Side, size: Optional[Tuple[int, int]]):
        self.order, self.side, self.size = _check_fields(order), side, size
        self._src: Optional[torch.Tensor] = None          # source frames [seen - len, seen): the context frame, then the ones not done
        self._todo = 0                                    # how many of them are not deinterlaced yet (they are the last ones)

    def push(self, frames: torch.Tensor) -> torch.Tensor:
        k = int(frames.shape[0])
        src = frames.contiguous() if self._src is None else torch.cat([self._src, frames], 0)
        n = int(src.shape[0])
        lo, hi = n - self._todo - k, n - 1                # all but the last frame, whose next is not known yet
        res = _deinterlace_device(src, self.order, self.side, self.size, lo, max(hi, lo))
        if hi > lo:
            self._src, self._todo = src[max(hi - 1, 0):].clone(), 1          # (a copy of two frames: the chunk's storage is released)
        else:
            self._src, self._todo = src, self._todo + k
        return res

    @property
    def held(self) -> int:
        """Source frames on the device between pushes: at most two."""
        return 0 if self._src is None else int(self._src.shape[0])

    def finish(self) -> Optional[torch.Tensor]:
        src, self._src = self._src, None
        if src is None or self._todo == 0:          # nothing was pushed (or finish() ran before)
            return None
        n = int(src.shape[0])
        return _deinterlace_device(src, self.order, self.side, self.size, n - self._todo, n)


# ---- telecined film (savsr_amd/pulldown.py is the specification) -----------------------------------------------------------------------------
def _check_pulldown(pulldown, cycle, fields) -> Optional[str]:
    """pulldown is None or a field order; pulldown_cycle goes with it, and fields= does not."""
    from .pulldown import DEFAULT_CYCLE, check_cycle
    if pulldown is None:
        if isinstance(cycle, bool) or cycle != DEFAULT_CYCLE:
            raise ValueError(f"pulldown_cycle = {cycle!r} goes with pulldown=: it is the decimation cycle of the pulldown removal")
        return None
    from .deinterlace import check_order
    check_order(pulldown, "pulldown")
    if fields is not None:
        raise ValueError(f"pulldown = {pulldown!r} together with fields = {fields!r}: they are two answers to one question (telecined film, "
                         f"whose frames are recovered, or interlaced video, whose fields are interpolated); give one of them")
    check_cycle(cycle, "pulldown_cycle")
    return pulldown


def _field_scores_device(frames: torch.Tensor, order: str, side: Side, size: Optional[Tuple[int, int]], lo: int = 0, hi: Optional[int] = None) -> torch.Tensor:
    """savsr_video_field_scores_* on resident frames of the input side on the GPU: int64 [hi - lo, 2] there for source frames [lo, hi)
    (default: all), the previous frame taken among the resident ones and clamped there; enqueued on the current stream (no sync).  Every
    byte of packed frames, the Y plane of planar ones."""
    from . import _lib
    from .deinterlace import FIELD_ORDERS
    n, c, h, w = _field_frames(frames, side, size)
    hi = n if hi is None else hi
    frames = frames.contiguous()
    lib = _lib.load()
    oid = FIELD_ORDERS.index(order)
    with torch.cuda.device(frames.device):
        out = torch.empty(max(hi - lo, 0), 2, dtype=torch.int64, device=frames.device)
        if hi <= lo:
            return out
        st = torch.cuda.current_stream().cuda_stream
        if not size:
            _lib.check(lib.savsr_video_field_scores_u8(frames.data_ptr(), n, h * w * c, 0, h, w * c, oid, lo, hi, out.data_ptr(), st),
                       "savsr_video_field_scores_u8")
        elif side.depth == 8:
            _lib.check(lib.savsr_video_field_scores_u8(frames.data_ptr(), n, side.frame_bytes(h, w), 0, h, w, oid, lo, hi, out.data_ptr(), st),
                       "savsr_video_field_scores_u8")
        else:
            _lib.check(lib.savsr_video_field_scores_u16(frames.data_ptr(), n, side.frame_bytes(h, w), 0, h, w, side.depth, oid, lo, hi, out.data_ptr(), st),
                       "savsr_video_field_scores_u16")
    return out


def _weave_device(frames: torch.Tensor, order: str, delta: torch.Tensor, side: Side, size: Optional[Tuple[int, int]], lo: int = 0,
                  hi: Optional[int] = None) -> torch.Tensor:
    """savsr_video_weave on resident frames of the input side on the GPU: the hi - lo woven frames of source frames [lo, hi) (default:
    all) with the device table delta (int32 [hi - lo], -1 | 0).  One call per plane, on the current stream."""
    from . import _lib
    from .deinterlace import FIELD_ORDERS
    n, c, h, w = _field_frames(frames, side, size)
    hi = n if hi is None else hi
    frames = frames.contiguous()
    out = frames.new_empty((max(hi - lo, 0),) + tuple(frames.shape[1:]))
    if hi <= lo:
        return out
    if delta.dtype != torch.int32 or delta.device != frames.device or delta.numel() != hi - lo or not delta.is_contiguous():
        raise ValueError(f"delta must be {hi - lo} contiguous int32 on {frames.device}, got {delta.dtype} {tuple(delta.shape)} on {delta.device}")
    lib = _lib.load()
    oid = FIELD_ORDERS.index(order)
    with torch.cuda.device(frames.device):
        st = torch.cuda.current_stream().cuda_stream
        if not size:
            table = [(0, h, w * c)]
            fb = h * w * c
        else:
            table = [t[:3] for t in _plane_table(h, w, side)]
            fb = side.frame_bytes(h, w)
        for off, ph, pb in table:
            _lib.check(lib.savsr_video_weave(frames.data_ptr(), n, fb, off, ph, pb, oid, lo, hi, delta.data_ptr(), out.data_ptr(), fb, off, st),
                       "savsr_video_weave")
    return out


def field_scores(frames: torch.Tensor, order: str, pixel_format: str = "rgb", size=None, depth: int = 8) -> torch.Tensor:
    """The field matcher's scores: int64 [N, 2] on the GPU (savsr_amd.pulldown.frame_scores is the specification, bit for bit), on the
    caller's current stream, without a sync.  Entry [n, j] is the comb measure of frame n with its second field (the rows of the other
    parity than `order`'s first field) taken from frame max(n - 1, 0) (j = 0) or from itself (j = 1).  frames as for `deinterlace`:
    [N, h, w, c] uint8 (every byte), or planar frames with pixel_format=, size=(h, w) (the Y plane; at depth 10 / 12 a sample's 8 most
    significant bits).  Float frames are refused."""
    from .deinterlace import check_order
    check_order(order)
    side, size = _sad_side(pixel_format, size, depth)
    _field_frames(frames, side, size)
    return _field_scores_device(_to_device(frames, _sad_device(frames)), order, side, size)


def _delta_device(matches: List[int], device: torch.device) -> torch.Tensor:
    from ._xfer import h2d
    return h2d(torch.tensor(matches, dtype=torch.int32), device)


def _remove_pulldown_device(frames: torch.Tensor, order: str, side: Side, size: Optional[Tuple[int, int]], cycle: int):
    """pulldown.remove_pulldown_frames on frames of the input side on the GPU: (the kept woven frames, info).  Two host synchronisations:
    the scores come down for the match, the woven frames' pair SADs for the decimation."""
    from . import pulldown as pd
    n = _field_frames(frames, side, size)[0]
    if n < 1:
        raise ValueError("the video has no frames")
    scores = _field_scores_device(frames, order, side, size).cpu()
    matches = pd.matches_from_scores(scores.numpy())
    woven = _weave_device(frames, order, _delta_device(matches, frames.device), side, size)
    sad = [-1] + _pair_sad_device(woven, side, size).cpu().tolist()
    kept = pd.kept_from_drops(n, pd.drops_from_sad(sad, cycle))
    out = woven.index_select(0, torch.tensor(kept, dtype=torch.int64).to(woven.device))
    return out, {"scores": scores.numpy(), "matches": matches, "sad": torch.tensor(sad, dtype=torch.int64).numpy(), "kept": kept}


def remove_pulldown(frames: torch.Tensor, order: str, pixel_format: str = "rgb", size=None, depth: int = 8, cycle: int = 5, return_info: bool = False):
    """Telecined film (3:2 pulldown) as its film frames: N - N // cycle frames on the GPU in the format of the N given ones
    (savsr_amd.pulldown.remove_pulldown_frames is the specification, bit for bit).  Every frame keeps its first field (order "tff": the
    top rows) and takes the second one from itself or from the frame before it, whichever combs less (`field_scores`); of every `cycle`
    woven frames the one closest to its predecessor (`pair_sad`) is dropped.  frames as for `deinterlace`.  return_info=True: (frames,
    info), info = {"scores", "matches", "sad", "kept"} as in the specification.  Two host synchronisations per call."""
    from .deinterlace import check_order
    from .pulldown import check_cycle
    check_order(order)
    cycle = check_cycle(cycle)
    side, size = _sad_side(pixel_format, size, depth)
    _field_frames(frames, side, size)
    out, info = _remove_pulldown_device(_to_device(frames, _sad_device(frames)), order, side, size, cycle)
    return (out, info) if return_info else out


class PulldownRemover:
    """The streaming pulldown removal behind VideoUpscaler(pulldown=...): push(source frames on the GPU) returns the film frames that are
    final, finish() the partial last cycle whole (None if there is none).  The match is causal, so a pushed frame is woven at once, with
    the previous push's last source frame as its context; woven frames wait until their cycle of `cycle` is complete, then the kept ones
    go on.  Between pushes the device keeps one source frame, at most cycle - 1 woven frames and the last woven frame (the next SAD's
    predecessor): `held` <= cycle + 1, copies of their own, so that the chunk they came with is released.  Concatenated, the outputs are
    `remove_pulldown` on the whole video for any chunking; `info` has the matches and the kept indices so far."""

    def __init__(self, order: str, side: Side, size: Optional[Tuple[int, int]], cycle: int = 5):
        from .deinterlace import check_order
        from .pulldown import check_cycle
        check_order(order, "pulldown")
        self.order, self.side, self.size, self.cycle = order, side, size, check_cycle(cycle, "pulldown_cycle")
        self._ctx: Optional[torch.Tensor] = None           # the last source frame pushed
        self._last: Optional[torch.Tensor] = None          # the last woven frame
        self._pend: Optional[torch.Tensor] = None          # the woven frames of the incomplete cycle, frames [_base, seen)
        self._pend_sad: List[int] = []                     # their pair SADs with their predecessors
        self._base = 0
        self.seen = 0
        self.matches: List[int] = []
        self.kept: List[int] = []

    @property
    def held(self) -> int:
        """Frames on the device between pushes: at most cycle + 1."""
        return sum(0 if t is None else int(t.shape[0]) for t in (self._ctx, self._last, self._pend))

    @property
    def info(self) -> dict:
        return {"matches": list(self.matches), "kept": list(self.kept)}

    def push(self, frames: torch.Tensor) -> torch.Tensor:
        from . import pulldown as pd
        k = int(frames.shape[0])
        if k == 0:
            return frames
        src = frames.contiguous() if self._ctx is None else torch.cat([self._ctx, frames], 0)
        n = int(src.shape[0])
        matches = pd.matches_from_scores(_field_scores_device(src, self.order, self.side, self.size, n - k, n).cpu().numpy())
        woven = _weave_device(src, self.order, _delta_device(matches, src.device), self.side, self.size, n - k, n)
        pairs = woven if self._last is None else torch.cat([self._last, woven], 0)
        sad = _pair_sad_device(pairs, self.side, self.size).cpu().tolist()
        self._pend_sad += ([-1] if self._last is None else []) + sad
        pend = woven if self._pend is None else torch.cat([self._pend, woven], 0)
        self.matches += matches
        self.seen += k
        full = (int(pend.shape[0]) // self.cycle) * self.cycle
        drops = set(pd.drops_from_sad(self._pend_sad[:full], self.cycle, self._base))
        kept = [j for j in range(self._base, self._base + full) if j not in drops]
        out = pend.index_select(0, torch.tensor([j - self._base for j in kept], dtype=torch.int64).to(pend.device))
        self.kept += kept
        self._pend = pend[full:].clone() if full < int(pend.shape[0]) else None
        self._pend_sad = self._pend_sad[full:]
        self._base += full
        self._ctx, self._last = src[n - 1:].clone(), woven[k - 1:].clone()
        return out

    def finish(self) -> Optional[torch.Tensor]:
        pend, self._pend, self._ctx, self._last = self._pend, None, None, None
        if pend is None:
            return None
        self.kept += list(range(self._base, self._base + int(pend.shape[0])))
        self._base += int(pend.shape[0])
        self._pend_sad = []
        return pend


def upscale_video(net, frames: torch.Tensor, scale=None, padding: str = "reflection", out: str = "float", pixel_format: str = "rgb",
                  size=None, cuts: Union[None, str, Sequence[int]] = None, scene_threshold=10.0, colour: str = "bt601",
                  out_colour: Optional[str] = None, depth: int = 8, out_depth: Optional[int] = None, siting: Optional[str] = None,
                  out_siting: Optional[str] = None, chroma_filter: Optional[str] = None, crop=None, crop_limit=24,
                  bars: str = "keep", fields: Optional[str] = None, pulldown: Optional[str] = None, pulldown_cycle: int = 5) -> torch.Tensor:
    """SAVSR.upscale_video (see there)."""
    _check_net(net)
    check_padding(padding)
    spec = video_spec(net.cfg["num_in_ch"], out, pixel_format, size, colour, out_colour, depth, out_depth, siting, out_siting, chroma_filter)
    sc = as_scale(net.scale if scale is None else scale)
    n, h, w = spec.frames_hw(frames)
    if _check_fields(fields) is not None:          # everything below sees the progressive video of 2N frames
        _field_frames(frames, spec.inp, spec.size)
        n *= 2
    if _check_pulldown(pulldown, pulldown_cycle, fields) is not None:          # everything below sees the film of N - N // cycle frames
        _field_frames(frames, spec.inp, spec.size)
        n -= n // pulldown_cycle
    crop = _check_crop_args(crop, crop_limit, bars)
    if crop is not None and crop != "auto":
        from . import active
        crop = active.check_rect(crop, h, w, spec.inp.layout)
    T = net.num_frame
    if cuts is None:
        check_length(n, T, padding)
    else:
        from . import scenes
        check_cuts_arg(cuts)
        scenes.check_threshold(scene_threshold)
        if n < 1:
            raise ValueError("the video has no frames")
        if not _is_auto(cuts):
            cuts = scenes.check_cuts(cuts, n)
    dev = net.gamma.device
    if dev.type != "cuda":
        raise RuntimeError("savsr_amd runs on an AMD GPU only: move the network to the GPU (net.cuda()) first")
    frames = _to_device(frames, dev)
    if fields is not None:             # deinterlacing comes first, before the crop
        frames = _deinterlace_device(frames, fields, spec.inp, spec.size)
    if pulldown is not None:           # pulldown removal comes first, where deinterlacing comes
        frames = _remove_pulldown_device(frames, pulldown, spec.inp, spec.size, pulldown_cycle)[0]
    full = spec
    if crop == "auto":
        crop = _detect_device(frames, spec.inp, spec.size, crop_limit)
    if crop == (0, 0, h, w):          # the whole frame: the uncropped path
        crop = None
    if crop is not None:               # the crop comes first: everything below sees the cropped video
        frames = _crop_device(frames, crop, spec.inp, (h, w))
        spec = _cropped_spec(spec, crop)
    if cuts is None:
        windows = [window_indices(i, n, T, padding) for i in range(n)]
    else:
        if _is_auto(cuts):
            sad = _pair_sad_device(frames, spec.inp, spec.size).cpu().tolist()
            cuts = scenes.cuts_from_sad(sad, scenes.sad_samples(frames.shape, pixel_format, spec.size), scene_threshold)
        windows = scenes.scene_windows(n, cuts, T, padding)
    with torch.no_grad():
        res = net.engine().forward_video(frames, windows, sc, spec, ensemble=net.self_ensemble)
        if crop is not None and bars == "keep":
            from . import active
            res = _insert_device(res, active.place(crop, h, w, sc, full.out.layout), full)
        return res


class VideoUpscaler:
    """Streaming form of SAVSR.upscale_video for long videos and decoders:

        up = VideoUpscaler(net, scale=4, padding="reflection", out="uint8")
        for chunk in decoder:                 # [k, h, w, c] uint8 (host or GPU) or [k, c, h, w] float on the GPU;
                                              # with pixel_format="i420", size=(h, w): [k, i420_bytes(h, w)] uint8
            emit(up.push(chunk))              # the SR frames whose windows are complete
        emit(up.finish())                     # the rest (with reflection the last num_frame // 2 need the end of the video)

    Concatenated, the outputs are bit for bit upscale_video on the whole video, for any chunking (a frame's output depends on its
    window only).  The network's self-ensemble switch is read once, here, like the scale.  The device keeps the past frames a later
    window may still name -- at most num_frame - 1 (num_frame for the two circle modes, whose last windows reach num_frame - 1 frames
    back) -- plus the current chunk.

    colour / out_colour: the colour spaces of I420 chunks in / out, as in upscale_video.  depth / out_depth: their bit depths (10, 12:
    chunks of [k, 2 * i420_bytes(h, w)] uint8, 16-bit samples), as in upscale_video.  pixel_format / out = "i422", "i444": chunks of
    [k, yuv.frame_bytes(h, w, depth, chroma)] uint8 in those layouts, as in upscale_video.  siting / out_siting: the chroma siting of YUV
    chunks in / out, as in upscale_video.

    cuts=[k, ...] (global frame indices) or cuts="auto" (each push scores its new pairs on the device, the pair with the previous
    push's last frame included, and decides with `scene_threshold`): windows stop at cuts as in upscale_video(cuts=...), and `up.cuts`
    lists the cuts among the frames pushed so far.  A frame is returned once its window is the same however the video continues -- a cut
    may still come anywhere after the last pushed frame (savsr_amd.scenes.ScenePlan); the frames kept are bounded as without cuts.

    crop=(y0, x0, ah, aw), bars="keep" / "drop": as in upscale_video, with an explicit rect only ("auto" needs the whole video: detect
    first with savsr_amd.detect_active_area).  Chunks are checked against the full frame size and cropped as they arrive, so the device
    buffer holds cropped frames; `spec` is the VideoSpec of the cropped size.

    fields="tff" / "bff": interlaced chunks, as in upscale_video.  Every source frame becomes two progressive frames as soon as the frame
    after it has been pushed (its second field reads that frame), so push() holds the last source frame back and finish() flushes it with
    next = cur; the cuts, the crop and the windows operate on the progressive frames as they are produced, and explicit cuts index them.
    Concatenated, the outputs are upscale_video(fields=...) on the whole video for any chunking.  Beside the frames kept without fields
    the device keeps at most two more source frames between pushes: the held frame and the one before it (savsr_amd.video.FieldSplitter).

    pulldown="tff" / "bff", pulldown_cycle=5: telecined chunks, as in upscale_video.  The match is causal, so a pushed frame is woven at
    once; woven frames wait until their cycle is complete, then the kept ones go on as a chunk and finish() flushes the partial last cycle
    whole.  Concatenated, the outputs are upscale_video(pulldown=...) on the whole video for any chunking; `pulldown_info` has the matches
    and the kept indices so far.  Beside the frames kept without it the device keeps at most pulldown_cycle + 1 more frames between pushes
    (savsr_amd.video.PulldownRemover).  Two host synchronisations per push."""

    def __init__(self, net, scale=None, padding: str = "reflection", out: str = "float", pixel_format: str = "rgb", size=None,
                 cuts: Union[None, str, Sequence[int]] = None, scene_threshold=10.0, colour: str = "bt601", out_colour: Optional[str] = None,
                 depth: int = 8, out_depth: Optional[int] = None, siting: Optional[str] = None, out_siting: Optional[str] = None,
                 chroma_filter: Optional[str] = None, crop=None, bars: str = "keep", fields: Optional[str] = None, pulldown: Optional[str] = None,
                 pulldown_cycle: int = 5):
        _check_net(net)
        check_padding(padding)
        check_out(out, net.cfg["num_in_ch"], chroma_filter)          # (speaks before the cuts, video_spec after them: the order of refusals)
        self._plan = None                          # scenes.ScenePlan when cuts are given; None: the path without cuts, as it was
        if cuts is not None:
            from . import scenes
            check_cuts_arg(cuts)
            self._threshold = scenes.check_threshold(scene_threshold)
            self._auto = _is_auto(cuts)
            self._given = [] if self._auto else scenes.check_cuts(cuts, None)       # explicit cuts not reached yet
            self._prev_sad = 0                     # the last pair's score (scdet's damping term), carried from push to push
            self._plan = scenes.ScenePlan(net.num_frame, padding)
        # the frames on both sides, checked once, here; the luma-only path (`luma_mode`) is decided with them
        self.spec = video_spec(net.cfg["num_in_ch"], out, pixel_format, size, colour, out_colour, depth, out_depth, siting, out_siting, chroma_filter)
        self._full = self.spec                     # the spec of the chunks as pushed; `spec` becomes the cropped size's with a crop
        self._split = None if _check_fields(fields) is None else FieldSplitter(fields, self.spec.inp, self.spec.size)          # None: as it was
        if _check_pulldown(pulldown, pulldown_cycle, fields) is not None:          # (the two exclude each other: one stage in front of the rest)
            self._split = PulldownRemover(pulldown, self.spec.inp, self.spec.size, pulldown_cycle)
        self._rect = _check_crop_args(crop, 24, bars, auto_ok=False)          # the rect to crop every chunk to; None: no crop, as it was
        self._place = None                         # active.place's six numbers with bars="keep", once the frame size is known
        self.bars = bars
        if self._rect is not None and self.spec.size:
            self._set_rect(*self.spec.size)
        self.i420 = self.spec.size                 # (h, w) of the planar frames the engine sees, None for packed ones
        self.net, self.padding, self.out = net, padding, out
        self.scale = as_scale(net.scale if scale is None else scale)
        self.ensemble = net.self_ensemble          # (read once, like the scale: every chunk runs the same flow)
        self.T = net.num_frame
        self.half = self.T // 2
        self._buf: Optional[torch.Tensor] = None      # frames [base, seen) on the device
        self._base = 0                                # video index of _buf[0]
        self.seen = 0                                 # frames pushed
        self.done = 0                                 # frames returned
        self._shape: Optional[tuple] = None           # (dtype is uint8, h, w)
        self._finished = False

    def _set_rect(self, h: int, w: int) -> None:
        """The rect against the full frame size, known now: refused if it does not fit; the whole frame is the uncropped path."""
        from . import active
        rect = active.check_rect(self._rect, h, w, self._full.inp.layout)
        if rect == (0, 0, h, w):
            self._rect = None
            return
        self._rect, self._hw = rect, (h, w)
        self.spec = _cropped_spec(self._full, rect)

    @property
    def pulldown_info(self) -> Optional[dict]:
        """{"matches", "kept"} of the frames pushed so far: per source frame -1 (its second field came from its predecessor) or 0, and the
        indices of the woven frames that went on (None without pulldown=)."""
        return self._split.info if isinstance(self._split, PulldownRemover) else None

    @property
    def cuts(self) -> Optional[List[int]]:
        """The cuts among the frames pushed so far (None without cuts=)."""
        return None if self._plan is None else list(self._plan.cuts)

    def _ready(self, i: int) -> bool:
        """Frame i's window is known whatever the video's length turns out to be (>= seen)."""
        if i + self.half >= self.seen:
            return False
        return max(window_indices(i, i + self.half + 1, self.T, self.padding)) < self.seen

    def _keep_from(self) -> int:
        """Oldest frame a window not returned yet may name, for every length the video can still have."""
        lo = self.seen
        for i in range(self.done, self.seen + self.half + 1):
            for n in range(max(self.seen, i + 1), max(self.seen, i + 1) + self.half + 1):
                lo = min(lo, min(window_indices(i, n, self.T, self.padding)))
        return max(lo, 0)

    def _forward(self, windows: List[List[int]]) -> torch.Tensor:
        """The SR frames of windows into the buffered frames."""
        with torch.no_grad():
            res = self.net.engine().forward_video(self._buf, windows, self.scale, self.spec, ensemble=self.ensemble)
            if self._rect is not None and self.bars == "keep":
                from . import active
                res = _insert_device(res, active.place(self._rect, *self._hw, self.scale, self._full.out.layout), self._full)
            return res

    def _run(self, upto: int, n_total: Optional[int]) -> torch.Tensor:
        """SR frames [done, upto); windows at the video length n_total (None: not known yet, every window needed is interior)."""
        n = n_total if n_total is not None else upto + self.half + 1
        res = self._forward([[j - self._base for j in window_indices(i, n, self.T, self.padding)] for i in range(self.done, upto)])
        self.done = upto
        return res

    def push(self, frames: torch.Tensor) -> torch.Tensor:
        if self._finished:
            raise RuntimeError("push() after finish()")
        if self._split is not None:                # interlaced / telecined chunks: the progressive frames that are final go on as a chunk of their own
            _field_frames(frames, self._full.inp, self._full.size)
            k, h, w = self._full.frames_hw(frames)
            dev = self.net.gamma.device
            if dev.type != "cuda":
                raise RuntimeError("savsr_amd runs on an AMD GPU only: move the network to the GPU (net.cuda()) first")
            if self._shape is not None and (True, h, w) != self._shape:
                raise ValueError(f"chunk of uint8 {h} x {w} frames after uint8 {self._shape[1]} x {self._shape[2]} ones")
            frames = self._split.push(_to_device(frames, dev))
            if int(frames.shape[0]) == 0:          # (a first push of one frame, or a cycle not complete yet: nothing is final)
                if self._shape is None and self._rect is not None and not self._full.size:
                    self._set_rect(h, w)
                self._shape = (True, h, w)
                return self._empty()
        return self._push(frames)

    def _push(self, frames: torch.Tensor) -> torch.Tensor:
        k, h, w = self._full.frames_hw(frames)
        shape = (frames.dtype == torch.uint8, h, w)
        if self._shape is not None and shape != self._shape:
            raise ValueError(f"chunk of {'uint8' if shape[0] else 'float'} {h} x {w} frames after {'uint8' if self._shape[0] else 'float'} "
                             f"{self._shape[1]} x {self._shape[2]} ones")
        if self._shape is None and self._rect is not None and not self._full.size:
            self._set_rect(h, w)                   # (packed chunks carry the frame size: the rect is checked against the first one's)
        dev = self.net.gamma.device
        if dev.type != "cuda":
            raise RuntimeError("savsr_amd runs on an AMD GPU only: move the network to the GPU (net.cuda()) first")
        self._shape = shape
        new = _to_device(frames, dev)
        new = new.contiguous() if shape[0] else new.to(torch.float32).contiguous()
        if self._rect is not None:
            new = _crop_device(new, self._rect, self._full.inp, (h, w))
        self._buf = new if self._buf is None else torch.cat([self._buf, new], 0)
        if self._plan is not None:
            return self._push_scenes(k)
        self.seen += k
        upto = self.done
        while upto < self.seen and self._ready(upto):
            upto += 1
        res = self._run(upto, None) if upto > self.done else self._empty()
        lo = self._keep_from()
        if lo > self._base:
            self._buf = self._buf[lo - self._base:]        # (a view: the next push's cat copies it)
            self._base = lo
        return res

    def _new_cuts(self, k: int) -> List[int]:
        """The cuts among the k frames just appended to the buffer."""
        lo, hi = self.seen, self.seen + k
        if not self._auto:
            n = sum(1 for c in self._given if c < hi)
            new, self._given = self._given[:n], self._given[n:]
            return new
        first = max(lo, 1)                          # frame `first`'s pair starts at the previous push's last frame, still in the buffer
        if hi - first < 1:
            return []
        from .scenes import cuts_from_sad, sad_samples
        sad = _pair_sad_device(self._buf[first - 1 - self._base:], self.spec.inp, self.i420).cpu().tolist()
        new = cuts_from_sad(sad, sad_samples(self._buf.shape, self.spec.inp.fmt, self.i420), self._threshold, first, self._prev_sad)
        self._prev_sad = sad[-1]
        return new

    def _run_windows(self, windows: List[List[int]]) -> torch.Tensor:
        return self._forward([[j - self._base for j in win] for win in windows]) if windows else self._empty()

    def _push_scenes(self, k: int) -> torch.Tensor:
        plan = self._plan
        plan.push(k, self._new_cuts(k))
        self.seen = plan.seen
        res = self._run_windows(plan.take())
        self.done = plan.done
        lo = plan.keep_from()
        if self._auto:
            lo = min(lo, self.seen - 1)            # the next push's first pair
        if lo > self._base:
            self._buf = self._buf[lo - self._base:]
            self._base = lo
        return res

    def finish(self) -> torch.Tensor:
        if self._finished:
            raise RuntimeError("finish() called twice")
        self._finished = True
        last = None if self._split is None else self._split.finish()          # the held source frame's two fields, then the end as ever
        if last is not None:
            head = self._push(last)
            return torch.cat([head, self._finish()], 0)
        return self._finish()

    def _finish(self) -> torch.Tensor:
        if self.seen == 0:
            raise ValueError("the video has no frames")
        if self._plan is not None:
            if self._given:
                raise ValueError(f"cut {self._given[0]}: a cut is the first frame of a new scene, 0 < k < {self.seen}")
            self._plan.end()
            res = self._run_windows(self._plan.take())
            self.done = self._plan.done
            self._buf = None
            return res
        check_length(self.seen, self.T, self.padding)
        res = self._run(self.seen, self.seen) if self.done < self.seen else self._empty()
        self._buf = None
        return res

    def _empty(self) -> torch.Tensor:
        from .packing import get_hw
        u8, h, w = self._shape
        if self._rect is not None and self.bars == "drop":
            h, w = self._rect[2:]
        H, W = get_hw(h, w, self.scale)
        c = self.net.cfg["num_in_ch"]
        dev = self.net.gamma.device
        if self.spec.out_kind == "planar":
            return torch.empty(0, self.spec.out.frame_bytes(H, W), dtype=torch.uint8, device=dev)
        if self.spec.out_kind == "uint8":
            return torch.empty(0, H, W, c, dtype=torch.uint8, device=dev)
        return torch.empty(0, c, H, W, dtype=torch.float32, device=dev)


def window_lists(n: int, num_frame: int, padding: str) -> List[List[int]]:
    """Every frame's window of an n-frame video (generate_frame_indices)."""
    check_padding(padding)
    check_length(n, num_frame, padding)
    return [window_indices(i, n, num_frame, padding) for i in range(n)]
