"""Everything that runs on the device in front of the network: the scene detector's scores, the active-picture detector with crop and
re-insertion, the deinterlacer, the pulldown removal and the scan detector that chooses between the two -- and, at the very boundary, the surface conversion (`unpack_surface` in front of
all of them, `pack_surface` behind everything; savsr_amd/surface.py is its specification).  Each is a public call on any frames and a
`_..._device` form on resident frames of a checked input side (what upscale_video calls on the whole video); the two that change the frame count are streaming stages as well
(`FieldSplitter`, `PulldownRemover`; `make_stage` builds the one a call asks for; `ScanStats` is the detector's streaming form), and the temporal
denoiser behind them is a third (`denoise_video`, `TemporalDenoiser`, `make_denoiser`; savsr_amd/denoise.py is its specification); the spatial
denoiser behind the crop is stateless (`denoise_spatial`; savsr_amd/nlmeans.py is its specification), and so is the deblocking stage on the
frames as decoded, in front of all of these but the surface conversion and the scan detector (`deblock_video`; savsr_amd/deblock.py), with
the deringing stage right behind it (`dering_video`; savsr_amd/dering.py).  The
numpy modules (scenes.py, active.py, deinterlace.py, pulldown.py, scan.py) are the specifications, bit for bit.  Where the byte matrices of a frame lie is `frames.plane_table`'s
answer alone; fp32 CHW frames have entries of their own (`_f32`) and are one explicit branch in the two stages that accept them.
"""
from __future__ import annotations

from dataclasses import replace
from typing import List, Optional, Tuple

import torch

from . import active
from . import deblock as db
from . import denoise as dn
from . import dering as dr
from . import grid as gr
from . import nlmeans as nl
from . import noise as nz
from . import pulldown as pd
from . import scan as sc
from .deinterlace import DEINTERLACERS, FIELD_ORDERS, FIELD_RATES, check_frame_rows, check_method, check_order, check_rate
from .frames import SAMPLE_FORMATS, Side, VideoSpec, check_sample_alignment, detector_layout, detector_side, layout_of, plane_table
from .scenes import check_threshold, cuts_from_sad, sad_samples
from .surface import LAYOUTS, Surface, SurfaceTable, check_stride, check_surface, descriptor
from .yuv import CHROMAS

Size = Optional[Tuple[int, int]]


def _to_device(frames: torch.Tensor, device: torch.device) -> torch.Tensor:
    if frames.device == device:
        return frames
    if frames.is_cuda:
        raise RuntimeError(f"frames on {frames.device}, network on {device}")
    from ._xfer import h2d
    return h2d(frames.contiguous(), device)


def _sad_device(frames: torch.Tensor) -> torch.device:
    if frames.is_cuda:
        return frames.device
    if not torch.cuda.is_available():
        raise RuntimeError("savsr_amd runs on an AMD GPU only: the detector's scores are computed there")
    return torch.device("cuda", torch.cuda.current_device())


def _stage_args(frames: torch.Tensor, pixel_format: str, size, depth, layout=detector_layout):
    """What a public stage call hands its `_..._device` form: (the frames on the GPU, host ones copied there; the side; the size), after
    `layout` has refused the frames that are none of that side."""
    side, size = detector_side(pixel_format, size, depth)
    layout(frames, side, size)
    return _to_device(frames, _sad_device(frames)), side, size


# ---- video surfaces (savsr_amd/surface.py is the specification) ------------------------------------------------------------------------
def surface_table(surface: Surface, side: Side, hw: Tuple[int, int], what: str = "surface") -> SurfaceTable:
    """The table of `surface` for h x w frames of a planar side; refuses, by name, a side that is not planar and what `resolve` refuses."""
    surface_side(surface, side, what)
    return surface.resolve(hw[0], hw[1], side.depth, side.layout)


def surface_side(surface: Surface, side: Side, what: str = "surface") -> None:
    """`surface` (or `out_surface`) goes with a planar side: refuses, by name, anything but a Surface, and a side that is not planar."""
    check_surface(surface, what)
    if not side.planar:
        fmt = "pixel_format" if what == "surface" else "out"
        raise ValueError(f"{what} = Surface.{surface.kind}() goes with {fmt} = {', '.join(repr(f) for f in SAMPLE_FORMATS[:-1])} or "
                         f"{SAMPLE_FORMATS[-1]!r}: it says where planar samples lie; {side.fmt!r} frames have none")


def surface_layout(frames: torch.Tensor, tab: SurfaceTable) -> int:
    """N of surface frames: [N, stride] uint8 (GPU or host) with stride >= the surface's bytes; refuses anything else, naming both numbers."""
    if not isinstance(frames, torch.Tensor):
        raise TypeError(f"frames must be a torch.Tensor, got {type(frames).__name__}")
    if frames.dtype != torch.uint8 or frames.dim() != 2:
        raise ValueError(f"surface frames must be [N, bytes] uint8, got {frames.dtype} {tuple(frames.shape)}")
    check_stride(int(frames.shape[1]), tab, "surface frames")
    return int(frames.shape[0])


def _surface_call(entry: str, src: torch.Tensor, dst: torch.Tensor, tab: SurfaceTable, side: Side, hw: Tuple[int, int], *tail) -> None:
    """One of the two entries on resident frames, on the current stream: (source, n, its stride, h, w, depth, layout, msb, the planes,
    destination, its stride[, the surface's bytes])."""
    from . import _lib
    import ctypes as C
    lib = _lib.load()
    desc = descriptor(tab)
    with torch.cuda.device(src.device):
        _lib.check(getattr(lib, entry)(src.data_ptr(), int(src.shape[0]), int(src.shape[1]), hw[0], hw[1], side.depth, LAYOUTS.index(side.layout),
                                       int(tab.msb), desc.ctypes.data_as(C.POINTER(C.c_int64)), len(tab.planes), dst.data_ptr(), int(dst.shape[1]),
                                       *tail, torch.cuda.current_stream().cuda_stream), entry)


def _unpack_surface_device(frames: torch.Tensor, tab: SurfaceTable, side: Side, hw: Tuple[int, int]) -> torch.Tensor:
    """savsr_video_unpack_surface on surface frames [n, stride] on the GPU: the planar frames [n, side.frame_bytes(h, w)] there, one
    launch on the current stream (no sync)."""
    n = surface_layout(frames, tab)
    frames = frames.contiguous()
    check_sample_alignment(frames, side.depth, side.layout)
    out = torch.empty(n, side.frame_bytes(*hw), dtype=torch.uint8, device=frames.device)
    if n:
        _surface_call("savsr_video_unpack_surface", frames, out, tab, side, hw)
    return out


def _pack_surface_device(planar: torch.Tensor, tab: SurfaceTable, side: Side, hw: Tuple[int, int]) -> torch.Tensor:
    """savsr_video_pack_surface on planar frames [n, side.frame_bytes(h, w)] on the GPU: the surface frames [n, tab.bytes] there, every
    byte no sample maps to 0; one launch (after one memset when the surface is not tight) on the current stream (no sync)."""
    fb = side.frame_bytes(*hw)
    if planar.dtype != torch.uint8 or planar.dim() != 2 or int(planar.shape[1]) != fb:
        raise ValueError(f"planar frames of {hw[0]} x {hw[1]} are [N, {fb}] uint8, got {planar.dtype} {tuple(planar.shape)}")
    planar = planar.contiguous()
    check_sample_alignment(planar, side.depth, side.layout)
    out = torch.empty(int(planar.shape[0]), tab.bytes, dtype=torch.uint8, device=planar.device)
    if planar.shape[0]:
        _surface_call("savsr_video_pack_surface", planar, out, tab, side, hw, tab.bytes)
    return out


def _surface_args(frames, surface, pixel_format, size, depth):
    side, size = detector_side(pixel_format, size, depth)
    surface_side(surface, side)
    tab = surface_table(surface, side, size)
    if not isinstance(frames, torch.Tensor):
        raise TypeError(f"frames must be a torch.Tensor, got {type(frames).__name__}")
    return tab, side, size


def unpack_surface(frames: torch.Tensor, surface: Surface, pixel_format: str = "i420", size=None, depth: int = 8) -> torch.Tensor:
    """Frames in a video surface (NV12, P010, UYVY, pitched planar, ...: savsr_amd.surface.Surface) as the planar frames every other call
    takes: [N, frame_bytes(h, w, depth, layout)] uint8 on the GPU (savsr_amd.surface.unpack_frames is the specification, bit for bit),
    on the caller's current stream, without a sync.  frames: [N, stride] uint8, GPU or host (host frames are copied up as they are),
    stride >= the surface's bytes at size=(h, w); pixel_format ("i420", "i422", "i444", "y400") and depth name the samples, `surface`
    says where they lie."""
    tab, side, size = _surface_args(frames, surface, pixel_format, size, depth)
    surface_layout(frames, tab)
    return _unpack_surface_device(_to_device(frames, _sad_device(frames)), tab, side, size)


def pack_surface(planar: torch.Tensor, surface: Surface, pixel_format: str = "i420", size=None, depth: int = 8) -> torch.Tensor:
    """Planar frames [N, frame_bytes(h, w, depth, layout)] uint8 (GPU or host) in a video surface: [N, surface bytes] uint8 on the GPU
    (savsr_amd.surface.pack_frames is the specification, bit for bit), on the caller's current stream, without a sync.  Every byte no
    sample maps to is 0: row padding, padded lines, the low bits of msb words, the pad Y of an odd-width packed row."""
    tab, side, size = _surface_args(planar, surface, pixel_format, size, depth)
    detector_layout(planar, side, size)
    return _pack_surface_device(_to_device(planar, _sad_device(planar)), tab, side, size)


# ---- the scene detector (savsr_amd/scenes.py is the specification) ---------------------------------------------------------------------
def _pair_sad_device(frames: torch.Tensor, side: Side, size: Size) -> torch.Tensor:
    """savsr_video_pair_sad_* on frames of the input side already on the GPU: int64 [N - 1] there, enqueued on the current stream (no sync).
    Planar colour frames of every layout and depth are one entry (_yuvp: the Y plane), packed and grey-scale frames another (_u8)."""
    from . import _lib
    n, c, h, w = detector_layout(frames, side, size)
    lib = _lib.load()
    u8 = frames.dtype == torch.uint8
    frames = frames.contiguous() if u8 else frames.to(torch.float32).contiguous()
    with torch.cuda.device(frames.device):
        sad = torch.empty(n - 1, dtype=torch.int64, device=frames.device)
        st = torch.cuda.current_stream().cuda_stream
        if not u8:
            _lib.check(lib.savsr_video_pair_sad_f32(frames.data_ptr(), n, c, h, w, sad.data_ptr(), st), "savsr_video_pair_sad_f32")
        elif side.yuv:
            _lib.check(lib.savsr_video_pair_sad_yuvp(frames.data_ptr(), n, h, w, side.depth, CHROMAS.index(side.layout), sad.data_ptr(), st),
                       "savsr_video_pair_sad_yuvp")
        else:
            # grey-scale frames are [N, h, w, 1] frames of their samples' 8 most significant bits (host work only: no kernel of their own)
            if side.depth != 8:
                words = frames.view(torch.int16).to(torch.int32) & 0xFFFF
                frames = (words.clamp_(max=(1 << side.depth) - 1) >> (side.depth - 8)).to(torch.uint8)
            _lib.check(lib.savsr_video_pair_sad_u8(frames.data_ptr(), n, max(c, 1), h, w, sad.data_ptr(), st), "savsr_video_pair_sad_u8")
    return sad


def pair_sad(frames: torch.Tensor, pixel_format: str = "rgb", size=None, depth: int = 8) -> torch.Tensor:
    """The scene detector's scores: int64 [N - 1] on the GPU, entry j = the sum of absolute differences of the 8-bit samples of frames j
    and j + 1 (savsr_amd.scenes.pair_sad is the specification).  frames as for SAVSR.upscale_video, with any c in 1 .. 3: [N, h, w, c]
    uint8 (GPU or host; every byte), [N, c, h, w] float on the GPU (every value after the uint8 output's quantisation), or with
    pixel_format="i420", size=(h, w): [N, i420_bytes(h, w)] uint8 (the Y plane only).  depth = 10, 12 (I420 only): frames of 16-bit samples,
    [N, 2 * i420_bytes(h, w)] uint8, compared by their 8 most significant bits, so the scores keep the 8-bit scale.  pixel_format="i422" /
    "i444": frames of those layouts; the Y plane only, as for I420."""
    return _pair_sad_device(*_stage_args(frames, pixel_format, size, depth))


def detect_cuts(frames: torch.Tensor, threshold=10.0, pixel_format: str = "rgb", size=None, depth: int = 8) -> List[int]:
    """The scene cuts of a video: the frames k whose change from frame k - 1, damped by the previous pair's, is at least `threshold`
    per cent of the largest possible one (ffmpeg scdet's rule in exact integer arithmetic, savsr_amd.scenes.cuts_from_sad, on pair_sad's
    scores; one device -> host copy of N - 1 integers).  The default threshold is scdet's and is not validated on real footage."""
    check_threshold(threshold)
    sad = pair_sad(frames, pixel_format, size, depth)
    return cuts_from_sad(sad.cpu().tolist(), sad_samples(frames.shape, pixel_format, size), threshold)


# ---- the active picture (savsr_amd/active.py is the specification) ----------------------------------------------------------------------
def _line_sums_device(frames: torch.Tensor, side: Side, size: Size) -> Tuple[torch.Tensor, torch.Tensor]:
    """savsr_video_line_sums_* on frames of the input side already on the GPU: int64 ([N, h], [N, w]) there, enqueued on the current stream
    (no sync).  Every frame kind is host work over the three entries: which matrix, which stride, and the folding of their sums."""
    from . import _lib
    n, c, h, w = detector_layout(frames, side, size)
    lib = _lib.load()
    u8 = frames.dtype == torch.uint8
    frames = frames.contiguous() if u8 else frames.to(torch.float32).contiguous()
    with torch.cuda.device(frames.device):
        st = torch.cuda.current_stream().cuda_stream
        if u8:
            tab = plane_table(side, size, c, h, w)
            y = tab.planes[0]
            mats, width = n, y.row_bytes // tab.sample
        else:
            mats, width = n * c, w
        cells = torch.empty(mats * (h + width), dtype=torch.int32, device=frames.device)          # (one buffer: the entry zeroes it in one memset)
        rows, cols = cells[:mats * h].view(mats, h), cells[mats * h:].view(mats, width)
        if not u8:
            _lib.check(lib.savsr_video_line_sums_f32(frames.data_ptr(), n * c, h, w, rows.data_ptr(), cols.data_ptr(), st), "savsr_video_line_sums_f32")
            rows, cols = rows.view(n, c, h), cols.view(n, c, w)
        elif tab.sample == 2:
            _lib.check(lib.savsr_video_line_sums_u16(frames.data_ptr(), n, tab.stride, h, width, side.depth, rows.data_ptr(), cols.data_ptr(), st),
                       "savsr_video_line_sums_u16")
        else:
            _lib.check(lib.savsr_video_line_sums_u8(frames.data_ptr(), n, tab.stride, h, width, rows.data_ptr(), cols.data_ptr(), st),
                       "savsr_video_line_sums_u8")
            if c:
                cols = cols.view(n, w, c)          # (a cell is below 2^32: as int64 before the channels are folded)
        rows, cols = (t.to(torch.int64) & 0xFFFFFFFF for t in (rows, cols))          # the cells are unsigned
        if not u8:
            rows, cols = rows.sum(1), cols.sum(1)
        elif c:
            cols = cols.sum(2)
    return rows, cols


def line_sums(frames: torch.Tensor, pixel_format: str = "rgb", size=None, depth: int = 8) -> Tuple[torch.Tensor, torch.Tensor]:
    """The active-picture detector's line sums: int64 ([N, h], [N, w]) on the GPU, per frame the sum of the 8-bit samples of every row
    and of every column (savsr_amd.active.line_sums is the specification), on the caller's current stream, without a sync.  frames as for
    `pair_sad`, and the same samples: every byte of [N, h, w, c] uint8 frames (GPU or host), every value of [N, c, h, w] float frames on the
    GPU after the uint8 output's quantisation, the Y plane of planar frames (pixel_format=, size=(h, w); at depth 10 / 12 a sample's 8
    most significant bits)."""
    return _line_sums_device(*_stage_args(frames, pixel_format, size, depth))


def _detect_device(frames: torch.Tensor, side: Side, size: Size, limit) -> Tuple[int, int, int, int]:
    """The aligned active rect of frames of the input side on the GPU: the line sums, their maxima over the frames on the device, one
    device -> host copy of h + w integers, then active_rect and align_rect on the host."""
    n, c, h, w = detector_layout(frames, side, size)
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
    active.check_limit(limit)
    return _detect_device(*_stage_args(frames, pixel_format, size, depth), limit)


def _plane_views(frames: torch.Tensor, side: Side, hw: Tuple[int, int], rect):
    """Per plane of planar [n, frame_bytes] frames of h x w: (the rect's window of the plane as an [n, rows, bytes] view, the plane of
    the rect-sized frame in the table of that size).  rect = (y0, x0, ah, aw) in luma samples, divided by each plane's block; bytes, so
    a 16-bit sample is two of them and the offsets stay even."""
    y0, x0, ah, aw = rect
    n = frames.shape[0]
    tab = plane_table(side, hw)
    for p, q in zip(tab.planes, plane_table(side, (ah, aw)).planes):
        py, px = y0 // p.bv, (x0 // p.bh) * tab.sample
        yield frames[:, p.offset:p.offset + p.rows * p.row_bytes].view(n, p.rows, p.row_bytes)[:, py:py + q.rows, px:px + q.row_bytes], q


def _crop_device(frames: torch.Tensor, rect, side: Side, hw: Tuple[int, int]) -> torch.Tensor:
    """active.crop_frames on a device tensor: strided copies through views.  Planar frames: every plane sliced at the rect divided by its
    block and the slices concatenated."""
    y0, x0, ah, aw = rect
    if not side.planar:
        if frames.dtype == torch.uint8:
            return frames[:, y0:y0 + ah, x0:x0 + aw].contiguous()
        return frames[:, :, y0:y0 + ah, x0:x0 + aw].contiguous()
    return torch.cat([win.reshape(frames.shape[0], q.rows * q.row_bytes) for win, q in _plane_views(frames, side, hw, rect)], 1)


def _insert_device(sr: torch.Tensor, placed, spec: VideoSpec) -> torch.Tensor:
    """active.insert_frames on a device tensor: full-size frames of active.bars_frame with the picture's planes copied in at (Y0, X0)
    divided by each plane's block."""
    Hf, Wf, Ha, Wa, Y0, X0 = placed
    out, n = spec.out, sr.shape[0]
    bars = torch.from_numpy(active.bars_frame(Hf, Wf, out.fmt, out.depth, out.colour, spec.nch)).to(sr.device)
    full = bars.unsqueeze(0).repeat(n, *([1] * bars.dim()))
    if out.fmt == "float":
        full[:, :, Y0:Y0 + Ha, X0:X0 + Wa] = sr
    elif not out.planar:
        full[:, Y0:Y0 + Ha, X0:X0 + Wa] = sr
    else:
        for win, q in _plane_views(full, out, (Hf, Wf), (Y0, X0, Ha, Wa)):
            win[:] = sr[:, q.offset:q.offset + q.rows * q.row_bytes].view(n, q.rows, q.row_bytes)
    return full


def _check_crop_args(crop, crop_limit, bars, auto_ok: bool = True):
    """crop is None, "auto" or a rect; bars / crop_limit go with a crop.  The rect itself: active.check_rect, once the frame size is known."""
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


def _cropped_spec(spec: VideoSpec, rect) -> VideoSpec:
    """The VideoSpec of the cropped frames: the same sides at the rect's size."""
    return replace(spec, size=(rect[2], rect[3])) if spec.size else spec


# ---- interlaced video (savsr_amd/deinterlace.py is the specification) -----------------------------------------------------------------------
def _check_fields(fields) -> Optional[str]:
    if fields is None:
        return None
    check_order(fields, "fields")
    return fields


def _sample_frames(frames: torch.Tensor, side: Side, size: Size, verb: str = "deinterlace") -> Tuple[int, int, int, int]:
    """(N, c, h, w) of frames of integer samples (`detector_layout`'s, N = 0 allowed); refuses float frames, which the stage `verb`
    names cannot take."""
    if isinstance(frames, torch.Tensor) and not size and frames.is_floating_point():
        raise ValueError(f"float frames have no integer samples to {verb}: give [N, h, w, c] uint8 or planar frames (quantise first)")
    if isinstance(frames, torch.Tensor) and frames.dim() and int(frames.shape[0]) == 0:
        return (0,) + detector_layout(frames.new_zeros((1,) + tuple(frames.shape[1:])), side, size)[1:]
    return detector_layout(frames, side, size)


def _field_frames(frames: torch.Tensor, side: Side, size: Size) -> Tuple[int, int, int, int]:
    """(N, c, h, w) of frames the deinterlacer takes (`detector_layout`'s, N = 0 allowed); refuses float frames and frames whose matrices
    have one row."""
    n, c, h, w = _sample_frames(frames, side, size)
    check_frame_rows(h, side.layout)
    return n, c, h, w


def _field_job(frames: torch.Tensor, order: Optional[str], side: Side, size: Size, hi: Optional[int]):
    """What the field kernels' wrappers share: (the contiguous resident frames, their count, hi (default: all), the channels of
    packed frames (0: planar), the plane table, the order's id (None without an order))."""
    n, c, h, w = _field_frames(frames, side, size)
    return frames.contiguous(), n, n if hi is None else hi, c, plane_table(side, size, c, h, w), None if order is None else FIELD_ORDERS.index(order)


def _entry_call(name: str, frames: torch.Tensor, n: int, tab, p, head: tuple, tail: tuple) -> None:
    """One call of a matrix entry on the current stream (no sync): (frames, their count and stride, the plane's offset and rows, *head,
    *tail, the stream), the return code checked under the entry's name."""
    from . import _lib
    with torch.cuda.device(frames.device):
        _lib.check(getattr(_lib.load(), name)(frames.data_ptr(), n, tab.stride, p.offset, p.rows, *head, *tail, torch.cuda.current_stream().cuda_stream), name)


def _matrix_call(stem: str, frames: torch.Tensor, n: int, tab, p, side: Side, tail: tuple, step: Optional[int] = None, variant: str = "") -> None:
    """savsr_video_<stem>_u8<variant> or _u16<variant> on plane p, by the table's sample size.  The head is (row_bytes[, step]) for bytes --
    the step slot only on the entries that have one -- and (cols, depth) for 16-bit samples; `tail` is what follows it."""
    if tab.sample == 1:
        _entry_call(f"savsr_video_{stem}_u8{variant}", frames, n, tab, p, (p.row_bytes,) + (() if step is None else (step,)), tail)
    else:
        _entry_call(f"savsr_video_{stem}_u16{variant}", frames, n, tab, p, (p.row_bytes // 2, side.depth), tail)


def _check_table(table: torch.Tensor, name: str, count: int, device: torch.device) -> None:
    """A device table of the masked deinterlacer (flags) or the weave (delta): `count` contiguous int32 on the frames' device."""
    if table.dtype != torch.int32 or table.device != device or table.numel() != count or not table.is_contiguous():
        raise ValueError(f"{name} must be {count} contiguous int32 on {device}, got {table.dtype} {tuple(table.shape)} on {table.device}")


def _deinterlace_device(frames: torch.Tensor, order: str, side: Side, size: Size, lo: int = 0, hi: Optional[int] = None,
                        method: str = "yadif", rate: str = "double") -> torch.Tensor:
    """savsr_video_deinterlace_* on resident frames of the input side on the GPU: the 2 (hi - lo) progressive frames of source frames
    [lo, hi) (default: all), prev / next taken among the resident frames and clamped there.  One call per plane, on the current stream.
    method "bwdif" or rate "same" (hi - lo frames: the first field in time of every source frame, the others are not computed) go
    through the `_m` entries; the defaults run the entries they ran before."""
    mid, rid = DEINTERLACERS.index(method), FIELD_RATES.index(rate)
    frames, n, hi, c, tab, oid = _field_job(frames, order, side, size, hi)
    out = frames.new_empty(((1 if rid else 2) * max(hi - lo, 0),) + tuple(frames.shape[1:]))
    variant, extra = ("_m", (mid, rid)) if mid or rid else ("", ())
    for p in tab.planes if hi > lo else ():          # (the pixel step of packed frames is their channel count: neighbours of a sample are c bytes away)
        _matrix_call("deinterlace", frames, n, tab, p, side, (oid, lo, hi, out.data_ptr(), tab.stride, p.offset) + extra, max(c, 1), variant)
    return out


def deinterlace(frames: torch.Tensor, order: str, pixel_format: str = "rgb", size=None, depth: int = 8, method: str = "yadif",
                rate: str = "double") -> torch.Tensor:
    """Interlaced video as progressive frames at the field rate: 2N frames on the GPU in the format of the N given ones
    (savsr_amd.deinterlace.deinterlace_frames is the specification, bit for bit), on the caller's current stream, without a sync.  Output
    frame 2n + f keeps field f of source frame n (order "tff": the top field is the earlier one; "bff": the bottom one) and interpolates
    the other rows by ffmpeg yadif's rule.  frames: [N, h, w, c] uint8 (GPU or host, c in 1 .. 3), or with pixel_format "i420", "i422",
    "i444", "y400" and size=(h, w): [N, frame_bytes] uint8, every plane on its own, 16-bit samples at depth 10 / 12.  Float frames are
    refused, and so are frames of one row (three for 4:2:0: the chroma planes need two).  method="bwdif": the other rows by ffmpeg
    bwdif's rule (savsr_amd.deinterlace.bwdif_matrix), under which static video comes back as it is.  rate="same": N frames, the first
    field in time of every source frame (the frames [0::2] of the 2N; the others are not computed)."""
    check_order(order)
    check_method(method)
    check_rate(rate)
    frames, side, size = _stage_args(frames, pixel_format, size, depth, _field_frames)
    return _deinterlace_device(frames, order, side, size, method=method, rate=rate)


class _LookAhead:
    """The window of the streaming stages whose result for a frame needs the frame after it.  take(frames) appends the pushed frames and
    hands back (buffer, lo, hi): the frames [lo, hi) of `buffer` are final now -- all but the newest one, whose next frame is not known
    yet; take(None, last=True) hands back everything, the newest frame's next one clamped as at the end of the video, and (None, 0, 0)
    when nothing is left.  buffer[lo - 1] is the frame before the range where the video has one, buffer[hi] the frame after it where one
    was pushed.  Afterwards the window keeps that context frame and the frames not done yet, always as copies of its own, so that the
    chunk they came with is released: at most two frames once a range was handed back.
    ahead, behind (the temporal denoiser's radius; 1 and 1 above): a frame is final once `ahead` frames after it were pushed, and
    `behind` frames before the range stay as its context, where the video has them: at most ahead + behind frames between pushes
    (savsr_amd.denoise.stream_ranges is the numpy model of this indexing)."""

    def __init__(self, ahead: int = 1, behind: int = 1):
        self.ahead, self.behind = ahead, behind
        self.buf: Optional[torch.Tensor] = None          # the context frames (where there are any), then the frames not done yet
        self.todo = 0                                    # how many of them are not done yet (they are the last ones)

    @property
    def held(self) -> int:
        return 0 if self.buf is None else int(self.buf.shape[0])

    def take(self, frames: Optional[torch.Tensor], last: bool = False) -> Tuple[Optional[torch.Tensor], int, int]:
        k = 0 if frames is None else int(frames.shape[0])
        if self.buf is None:
            if frames is None:
                return None, 0, 0
            buf = frames.contiguous()
        else:
            buf = self.buf if frames is None else torch.cat([self.buf, frames], 0)
        n = int(buf.shape[0])
        lo = n - self.todo - k
        hi = n if last else max(n - self.ahead, lo)
        if last:
            self.buf, self.todo = None, 0
        elif hi > lo:
            self.buf, self.todo = buf[max(hi - self.behind, 0):].clone(), n - hi
        else:          # (nothing final yet: the pushed frames wait; a first push is the caller's storage and is copied)
            self.buf, self.todo = buf.clone() if self.buf is None else buf, self.todo + k
        return buf, lo, hi


class FieldSplitter:
    """The streaming deinterlacer behind VideoUpscaler(fields=...): push(source frames on the GPU) returns the progressive frames that are
    final, finish() the last source frame's two.  The second field of the last pushed frame needs the frame after it, so one source frame
    is held back; with the frame before it (the temporal context) the device keeps at most two source frames between pushes (copies of
    their own, so that the chunk they came with is released).  Concatenated, the outputs are `deinterlace` on the whole video for any
    chunking.  finish() without a pushed frame returns None.  method="bwdif" reads the same three frames, and with rate="same" the one
    field of a frame still reads the frame after it (its t2 term), so the same frame is held back for every method and rate."""

    def __init__(self, order: str, side: Side, size: Size, method: str = "yadif", rate: str = "double"):
        self.order, self.side, self.size = _check_fields(order), side, size
        check_method(method)
        check_rate(rate)
        self.method, self.rate = method, rate
        self._win = _LookAhead()

    def push(self, frames: torch.Tensor) -> torch.Tensor:
        src, lo, hi = self._win.take(frames)
        return _deinterlace_device(src, self.order, self.side, self.size, lo, hi, self.method, self.rate)

    @property
    def _src(self) -> Optional[torch.Tensor]:
        return self._win.buf

    @property
    def held(self) -> int:
        """Source frames on the device between pushes: at most two."""
        return self._win.held

    def finish(self) -> Optional[torch.Tensor]:
        src, lo, hi = self._win.take(None, True)
        if hi <= lo:          # nothing was pushed (or finish() ran before)
            return None
        return _deinterlace_device(src, self.order, self.side, self.size, lo, hi, self.method, self.rate)


# ---- temporal noise reduction (savsr_amd/denoise.py is the specification) ------------------------------------------------------------------
def _denoise_frames(frames: torch.Tensor, side: Side, size: Size) -> Tuple[int, int, int, int]:
    """(N, c, h, w) of frames the denoiser takes: what the deinterlacer takes, frames of one row included."""
    return _sample_frames(frames, side, size, "denoise")


def _denoise_device(frames: torch.Tensor, side: Side, size: Size, radius: int = dn.DEFAULT_RADIUS, strength=dn.DEFAULT_STRENGTH,
                    chroma_strength=None, lo: int = 0, hi: Optional[int] = None) -> torch.Tensor:
    """savsr_video_denoise_* on resident frames of the input side on the GPU: the hi - lo denoised frames of frames [lo, hi) (default:
    all), the taps taken among the resident frames, where the walks end.  One call per plane, on the current stream (no sync): the Y
    plane and the bytes of packed frames with `strength`, the chroma planes with `chroma_strength` (None: `strength`)."""
    n, c, h, w = _denoise_frames(frames, side, size)
    frames, hi, tab = frames.contiguous(), n if hi is None else hi, plane_table(side, size, c, h, w)
    out = frames.new_empty((max(hi - lo, 0),) + tuple(frames.shape[1:]))
    for i, p in enumerate(tab.planes if hi > lo else ()):
        a, b = strength if i == 0 or chroma_strength is None else chroma_strength
        _matrix_call("denoise", frames, n, tab, p, side, (radius, a, b, lo, hi, out.data_ptr(), tab.stride, p.offset))
    return out


def denoise_video(frames: torch.Tensor, pixel_format: str = "rgb", size=None, depth: int = 8, radius: int = dn.DEFAULT_RADIUS,
                  strength=dn.DEFAULT_STRENGTH, chroma_strength=None) -> torch.Tensor:
    """Temporal noise reduction: N frames on the GPU in the format of the N given ones (savsr_amd.denoise.denoise_frames is the
    specification, bit for bit), on the caller's current stream, without a sync.  Every sample becomes the rounded mean of itself and
    the same sample of up to `radius` frames on either side: two independent walks, each taking the next frame's sample while it
    differs by at most a and the walk's differences sum to at most b (ffmpeg atadenoise's serial rule; strength = (a, b) in 8-bit code
    units at every depth, 0 <= a <= b <= 255; 1 <= radius <= 16), ending at the video's ends.  frames as for `deinterlace`: [N, h, w, c]
    uint8 (GPU or host, every byte with `strength`), or with pixel_format "i420", "i422", "i444", "y400" and size=(h, w): [N, frame_bytes]
    uint8, every plane on its own, 16-bit samples at depth 10 / 12, the chroma planes with `chroma_strength` (None: `strength`).  Float
    frames are refused.  Static samples come back as they are, no sample moves by more than min(a, b) codes (shifted to the depth), and
    (0, 0) is the identity.  The defaults are parameters: nothing is validated on footage.  Temporal only: moving texture is not
    denoised, and the taps read across scene cuts, where only the thresholds stop them."""
    radius = dn.check_radius(radius)
    strength = dn.check_strength(strength)
    chroma_strength = None if chroma_strength is None else dn.check_strength(chroma_strength, "chroma_strength")
    frames, side, size = _stage_args(frames, pixel_format, size, depth, _denoise_frames)
    return _denoise_device(frames, side, size, radius, strength, chroma_strength)


class TemporalDenoiser:
    """The streaming denoiser behind VideoUpscaler(denoise=...): push(frames on the GPU) returns the denoised frames that are final --
    frame n once frame n + radius has been pushed -- and finish() the rest (None without a pushed frame).  Between pushes the device
    keeps at most 2 * radius frames: `radius` behind as context and `radius` not done yet, copies of their own, so that the chunk they
    came with is released.  Concatenated, the outputs are `denoise_video` on the whole video for any chunking."""

    def __init__(self, side: Side, size: Size, radius: int = dn.DEFAULT_RADIUS, strength=dn.DEFAULT_STRENGTH, chroma_strength=None):
        self.side, self.size = side, size
        self.radius, self.strength = dn.check_radius(radius), dn.check_strength(strength)
        self.chroma_strength = None if chroma_strength is None else dn.check_strength(chroma_strength, "chroma_strength")
        self._win = _LookAhead(self.radius, self.radius)

    @property
    def held(self) -> int:
        """Frames on the device between pushes: at most 2 * radius."""
        return self._win.held

    def _run(self, src: torch.Tensor, lo: int, hi: int) -> torch.Tensor:
        return _denoise_device(src, self.side, self.size, self.radius, self.strength, self.chroma_strength, lo, hi)

    def push(self, frames: torch.Tensor) -> torch.Tensor:
        return self._run(*self._win.take(frames))

    def finish(self) -> Optional[torch.Tensor]:
        src, lo, hi = self._win.take(None, True)
        if hi <= lo:          # nothing was pushed (or finish() ran before)
            return None
        return self._run(src, lo, hi)


def make_denoiser(denoise, radius, strength, chroma_strength, side: Side, size: Size) -> Optional[TemporalDenoiser]:
    """The streaming stage denoise= / denoise_radius= / denoise_strength= / denoise_chroma_strength= ask for, on frames of `side`, behind
    `make_stage`'s: None without denoise= (after `denoise.check_denoise_options` has refused options without it)."""
    opts = dn.check_denoise_options(denoise, radius, strength, chroma_strength)
    return None if opts is None else TemporalDenoiser(side, size, *opts)


# ---- spatial noise reduction (savsr_amd/nlmeans.py is the specification) --------------------------------------------------------------------
def _denoise_spatial_device(frames: torch.Tensor, side: Side, size: Size, patch: int = nl.DEFAULT_PATCH, search: int = nl.DEFAULT_SEARCH,
                            strength=nl.DEFAULT_STRENGTH, chroma_strength=None) -> torch.Tensor:
    """savsr_video_nlmeans_* on resident frames of the input side on the GPU: as many filtered frames, every frame on its own.  One call
    per plane, on the current stream (no sync): the Y plane with `strength`, the chroma planes with `chroma_strength` (None:
    `strength`); packed frames in one call, every channel a plane of its own (the channel count is the entry's sample step)."""
    n, c, h, w = _denoise_frames(frames, side, size)          # (what the temporal denoiser takes)
    frames, tab = frames.contiguous(), plane_table(side, size, c, h, w)
    out = torch.empty_like(frames)
    step = max(c, 1)
    for i, p in enumerate(tab.planes if n else ()):
        d = nl.divisor(patch, strength if i == 0 or chroma_strength is None else chroma_strength)
        head = (p.row_bytes // (tab.sample * step), step) + (() if tab.sample == 1 else (side.depth,))
        _entry_call("savsr_video_nlmeans_u8" if tab.sample == 1 else "savsr_video_nlmeans_u16", frames, n, tab, p, head,
                    (patch, search, d, out.data_ptr(), tab.stride, p.offset))
    return out


def denoise_spatial(frames: torch.Tensor, pixel_format: str = "rgb", size=None, depth: int = 8, patch: int = nl.DEFAULT_PATCH,
                    search: int = nl.DEFAULT_SEARCH, strength=nl.DEFAULT_STRENGTH, chroma_strength=None) -> torch.Tensor:
    """Spatial noise reduction (non-local means): N frames on the GPU in the format of the N given ones (savsr_amd.nlmeans.nlm_frames is
    the specification, bit for bit), on the caller's current stream, without a sync.  Every frame is filtered on its own: a sample
    becomes the weighted mean of the samples within `search` (1 .. 7) of it that lie inside the plane, each weighted by
    exp(-SSD / ((2 patch + 1)^2 h^2)) from a 577-entry integer table, SSD the squared difference of the (2 patch + 1)^2 patches
    (patch 1 .. 3) around the two, h = `strength` in 8-bit code units at every depth (0 < h <= 32).  frames as for `denoise_video`:
    [N, h, w, c] uint8 (GPU or host; every channel a plane of its own), or with pixel_format "i420", "i422", "i444", "y400" and
    size=(h, w): [N, frame_bytes] uint8, every plane on its own, 16-bit samples at depth 10 / 12, the chroma planes with
    `chroma_strength` (None: `strength`).  Float frames are refused.  A constant plane comes back as it is and every output lies
    within the range of its candidates.  The defaults (patch 3, search 7, strength 3.0) are parameters: nothing is validated on
    footage.  One strength per video, no joint-channel weights, no noise correction of the centre weight."""
    patch, search = nl.check_patch(patch), nl.check_search(search)
    nl.divisor(patch, strength)
    if chroma_strength is not None:
        nl.divisor(patch, chroma_strength, "chroma_strength")
    frames, side, size = _stage_args(frames, pixel_format, size, depth, _denoise_frames)
    return _denoise_spatial_device(frames, side, size, patch, search, strength, chroma_strength)


# ---- deblocking (savsr_amd/deblock.py is the specification) ----------------------------------------------------------------------------------
def _deblock_device(frames: torch.Tensor, side: Side, size: Size, block: int = db.DEFAULT_BLOCK, mode: str = "weak",
                    strength=db.DEFAULT_STRENGTH, chroma_strength=None, interlaced: bool = False, origin=(0, 0), chroma_origin=None) -> torch.Tensor:
    """savsr_video_deblock_* on resident frames of the input side on the GPU: as many filtered frames, every frame on its own.  One call
    (one launch, both passes in it) per plane, on the current stream (no sync): the Y plane with `strength`, the chroma planes with
    `chroma_strength` (None: `strength`), the thresholds shifted to the depth here; packed frames in one call, every channel a plane of
    its own (the channel count is the entry's sample step).  interlaced: every plane field by field.  origin / chroma_origin (None:
    the origin): the grid's origin in the Y plane's / the chroma planes' samples; a plane whose origin is (0, 0) goes through the entry
    it went through before, the others through the `_o` entries."""
    n, c, h, w = _sample_frames(frames, side, size, "deblock")
    frames, tab = frames.contiguous(), plane_table(side, size, c, h, w)
    out = torch.empty_like(frames)
    step, shift = max(c, 1), side.depth - 8
    for i, p in enumerate(tab.planes if n else ()):
        a, b = strength if i == 0 or chroma_strength is None else chroma_strength
        oy, ox = origin if i == 0 or chroma_origin is None else chroma_origin
        head = (p.row_bytes // (tab.sample * step), step) + (() if tab.sample == 1 else (side.depth,))
        tail = (block, int(mode == "strong"), int(bool(interlaced)), a << shift, b << shift, out.data_ptr(), tab.stride, p.offset)
        name = "savsr_video_deblock_u8" if tab.sample == 1 else "savsr_video_deblock_u16"
        if (oy, ox) != (0, 0):
            name, tail = name + "_o", tail + (int(oy), int(ox))
        _entry_call(name, frames, n, tab, p, head, tail)
    return out


def deblock_video(frames: torch.Tensor, pixel_format: str = "rgb", size=None, depth: int = 8, block: int = db.DEFAULT_BLOCK, mode: str = "weak",
                  strength=db.DEFAULT_STRENGTH, chroma_strength=None, interlaced: bool = False, origin=(0, 0), chroma_origin=None) -> torch.Tensor:
    """Deblocking: N frames on the GPU in the format of the N given ones (savsr_amd.deblock.deblock_frames is the specification, bit for
    bit), on the caller's current stream, without a sync.  Every frame is filtered on its own: across the vertical edges of a grid of
    `block` (4, 8 or 16) samples whose first edges lie at `origin` = (oy, ox), then across the horizontal ones, the samples next to an edge move
    towards each other by 1/2, (1/4,) 1/8 of the step across it -- 2 samples a side with mode "weak", 3 with "strong" -- where the step
    is below a and the steps beside it are below b, strength = (a, b) in 8-bit code units at every depth (ints in 0 .. 255).
    interlaced=True filters the two fields as planes of their own (vertical block `block` // 2, weak below 8, no vertical pass at block
    4), so that no filter mixes two moments.  frames as for `denoise_video`: [N, h, w, c] uint8 (GPU or host; every channel a plane of
    its own), or with pixel_format "i420", "i422", "i444", "y400" and size=(h, w): [N, frame_bytes] uint8, every plane on its own with
    the same block in its own samples, 16-bit samples at depth 10 / 12, the chroma planes with `chroma_strength` (None: `strength`).
    Float frames are refused.  A constant plane comes back as it is, a = 0 is the identity and a pass moves no sample by more than
    (a - 1) // 2 codes (shifted to the depth).  The defaults (block 8, (25, 13)) are parameters: nothing is validated on footage.
    origin = (oy, ox), 0 <= o < block (oy even with interlaced=True): a video cropped by c samples before it arrived has its edges at
    (-c) mod block; chroma_origin: the same for the Cb / Cr planes in chroma samples (None: the origin; 4:2:0 and 4:2:2 frames with
    an origin other than (0, 0) must name it).  `detect_grid` finds block and origins from the frames.  A video scaled before it
    arrives has no grid this stage knows."""
    block, mode = db.check_block(block), db.check_mode(mode)
    strength = db.check_strength(strength)
    chroma_strength = None if chroma_strength is None else db.check_strength(chroma_strength, "chroma_strength")
    origin, chroma_origin = db.check_origins(origin, chroma_origin, block, interlaced, layout_of(pixel_format) if size else None)
    frames, side, size = _stage_args(frames, pixel_format, size, depth, lambda f, s, z: _sample_frames(f, s, z, "deblock"))
    return _deblock_device(frames, side, size, block, mode, strength, chroma_strength, interlaced, origin, chroma_origin)


# ---- deringing (savsr_amd/dering.py is the specification) -----------------------------------------------------------------------------------
def _dering_device(frames: torch.Tensor, side: Side, size: Size, strength=dr.DEFAULT_STRENGTH, chroma_strength=None,
                   damping: int = dr.DEFAULT_DAMPING, interlaced: bool = False) -> torch.Tensor:
    """savsr_video_dering_* on resident frames of the input side on the GPU: as many filtered frames, every frame on its own.  One call
    (one launch) per plane, on the current stream (no sync): the Y plane with `strength`, the chroma planes with `chroma_strength`
    (None: `strength`), the strengths shifted to the depth here; packed frames in one call, every channel a plane of its own (the
    channel count is the entry's sample step).  interlaced: every plane field by field."""
    n, c, h, w = _sample_frames(frames, side, size, "dering")
    frames, tab = frames.contiguous(), plane_table(side, size, c, h, w)
    out = torch.empty_like(frames)
    step, shift = max(c, 1), side.depth - 8
    for i, p in enumerate(tab.planes if n else ()):
        pri, sec = strength if i == 0 or chroma_strength is None else chroma_strength
        head = (p.row_bytes // (tab.sample * step), step) + (() if tab.sample == 1 else (side.depth,))
        _entry_call("savsr_video_dering_u8" if tab.sample == 1 else "savsr_video_dering_u16", frames, n, tab, p, head,
                    (int(bool(interlaced)), pri << shift, sec << shift, damping, out.data_ptr(), tab.stride, p.offset))
    return out


def dering_video(frames: torch.Tensor, pixel_format: str = "rgb", size=None, depth: int = 8, strength=dr.DEFAULT_STRENGTH, chroma_strength=None,
                 damping: int = dr.DEFAULT_DAMPING, interlaced: bool = False) -> torch.Tensor:
    """Deringing: N frames on the GPU in the format of the N given ones (savsr_amd.dering.dering_frames is the specification, bit for
    bit), on the caller's current stream, without a sync.  Every frame is filtered on its own: every 8 x 8 block of a plane (the grid
    starts at the plane's origin) gets a direction from eight sets of line sums, and every sample moves by a constrained sum of four taps
    along its block's direction and eight across it -- strength = (p, s), 0 <= p <= 15 along (scaled by the block's directional
    variance; nothing on a flat block) and 0 <= s <= 4 across, damping 3 .. 6, all in 8-bit code units at every depth -- clamped to the
    minimum and maximum of the sample and its taps.  interlaced=True filters the two fields as planes of their own, each with its own
    blocks, so that no filter mixes two moments.  frames as for `deblock_video`: [N, h, w, c] uint8 (GPU or host; every channel a
    plane of its own), or with pixel_format "i420", "i422", "i444", "y400" and size=(h, w): [N, frame_bytes] uint8, every plane on its
    own, 16-bit samples at depth 10 / 12, the chroma planes with `chroma_strength` (None: `strength`).  Float frames are refused.  A
    constant plane comes back as it is, (0, 0) is the identity and no sample moves by more than (12 (p + s) + 8) >> 4 codes (shifted
    to the depth).  The defaults ((4, 2), damping 5) are parameters: nothing is validated on footage.  The grid does not follow a
    deblocker's origin, chroma gets a direction of its own, and the stage also smooths fine noise."""
    strength = dr.check_strength(strength)
    chroma_strength = None if chroma_strength is None else dr.check_strength(chroma_strength, "chroma_strength")
    damping = dr.check_damping(damping)
    frames, side, size = _stage_args(frames, pixel_format, size, depth, lambda f, s, z: _sample_frames(f, s, z, "dering"))
    return _dering_device(frames, side, size, strength, chroma_strength, damping, interlaced)


# ---- the block grid (savsr_amd/grid.py is the specification) --------------------------------------------------------------------------------
def _grid_stats_device(frames: torch.Tensor, side: Side, size: Size, interlaced: bool = False, cap: int = gr.DEFAULT_CAP) -> torch.Tensor:
    """savsr_video_grid_stats_* on resident frames of the input side on the GPU: int64 [N, 2, 2, 16] there (a view of [2, N, 2, 16]), one
    memset and one launch per plane on the current stream (no sync).  Class 0: the Y plane, or all channels of packed frames in one call (the channel count
    is the entry's sample step); class 1: the chroma planes, both added into the same cells."""
    n, c, h, w = _sample_frames(frames, side, size, "find a grid in")
    frames, tab = frames.contiguous(), plane_table(side, size, c, h, w)
    out = torch.zeros(2, n, 2, gr.CELLS, dtype=torch.int64, device=frames.device)          # by class: a class's frames are 32 cells apart, as the entry adds them
    step = max(c, 1)
    for i, p in enumerate(tab.planes if n else ()):
        head = (p.row_bytes // (tab.sample * step), step) + (() if tab.sample == 1 else (side.depth,))
        _entry_call("savsr_video_grid_stats_u8" if tab.sample == 1 else "savsr_video_grid_stats_u16", frames, n, tab, p, head,
                    (int(bool(interlaced)), cap, out[min(i, 1)].data_ptr()))
    return out.permute(1, 0, 2, 3)


def grid_stats(frames: torch.Tensor, pixel_format: str = "rgb", size=None, depth: int = 8, interlaced: bool = False,
               cap: int = gr.DEFAULT_CAP) -> torch.Tensor:
    """The grid detector's statistics: int64 [N, 2, 2, 16] on the GPU (savsr_amd.grid.grid_stats_frames is the specification, bit for
    bit), on the caller's current stream, without a sync.  [n, k, 0, x mod 16] counts, along the rows of class k of frame n, the
    boundaries whose step is larger than the two steps beside it together and at most `cap` (8-bit codes); [n, k, 1, y mod 16] the same
    along the columns, field by field with interlaced=True.  Class 0: the Y plane of planar frames, or every channel of [N, h, w, c]
    uint8 frames; class 1: Cb + Cr, zeros where there is none.  Float frames are refused.  cap is a parameter of this project's own:
    nothing is validated on footage."""
    cap = gr.check_cap(cap)
    frames, side, size = _stage_args(frames, pixel_format, size, depth, lambda f, s, z: _sample_frames(f, s, z, "find a grid in"))
    return _grid_stats_device(frames, side, size, interlaced, cap)


def _frame_pairs(frames: torch.Tensor, side: Side, size: Size, interlaced: bool):
    return gr.frame_pairs(tuple(frames.shape), side.fmt, size, side.depth, interlaced)


def _detect_grid_device(frames: torch.Tensor, side: Side, size: Size, interlaced: bool = False, ratio=gr.DEFAULT_RATIO,
                        min_count: int = gr.DEFAULT_MIN_COUNT, cap: int = gr.DEFAULT_CAP) -> "gr.GridVerdict":
    """grid.verdict_from_stats on `_grid_stats_device` of frames of the input side on the GPU, summed over the frames there: one device
    -> host copy of 64 integers."""
    n = _sample_frames(frames, side, size, "find a grid in")[0]
    table = _grid_stats_device(frames, side, size, interlaced, cap).sum(0).cpu().numpy()
    return gr.verdict_from_stats(table, n * _frame_pairs(frames, side, size, interlaced), interlaced, ratio, min_count)


def detect_grid(frames: torch.Tensor, pixel_format: str = "rgb", size=None, depth: int = 8, interlaced: bool = False, ratio=gr.DEFAULT_RATIO,
                min_count: int = gr.DEFAULT_MIN_COUNT, cap: int = gr.DEFAULT_CAP) -> "gr.GridVerdict":
    """The block grid of a video, from its content: a savsr_amd.grid.GridVerdict with block = 4, 8, 16 or None (no grid), origin =
    (oy, ox) and chroma_origin (None where the chroma planes show no grid of the luma's block); `verdict.kwargs()` is the explicit
    argument set of upscale_video / VideoUpscaler beside deblock= that says the same, {} without a grid.  `grid_stats` on the GPU summed
    over the frames, one host synchronisation, then savsr_amd.grid.verdict_from_stats in exact arithmetic: a cell of the 16 is a peak
    where it holds at least `min_count` hits and its hit rate is at least `ratio` times the median rate, and the peaks must be exactly
    those of one block size in both directions.  interlaced=True reads the columns field by field, as the deblocker will filter them.
    The rule and its defaults are this project's own and are not validated on footage; one grid per video; grids of scaled video,
    other block sizes and block 4 on noise-free material are not found; periodic picture content can fake a grid."""
    ratio, min_count, cap = gr.check_ratio(ratio), gr.check_min_count(min_count), gr.check_cap(cap)
    frames, side, size = _stage_args(frames, pixel_format, size, depth, lambda f, s, z: _sample_frames(f, s, z, "find a grid in"))
    return _detect_grid_device(frames, side, size, interlaced, ratio, min_count, cap)


# ---- the noise level (savsr_amd/noise.py is the specification) ------------------------------------------------------------------------------
def _noise_frames(frames: torch.Tensor, side: Side, size: Size) -> Tuple[int, int, int, int]:
    return _sample_frames(frames, side, size, "measure noise in")


def _noise_stats_device(frames: torch.Tensor, side: Side, size: Size, interlaced: bool = False) -> torch.Tensor:
    """savsr_video_noise_stats_* on resident frames of the input side on the GPU: int64 [N, 2, 256, 2] there (a view of [2, N, 256, 2]),
    one memset and one launch per plane on the current stream (no sync).  Class 0: the Y plane, or all channels of packed frames in one
    call (the channel count is the entry's sample step); class 1: the chroma planes, both added into the same table."""
    n, c, h, w = _noise_frames(frames, side, size)
    frames, tab = frames.contiguous(), plane_table(side, size, c, h, w)
    out = torch.zeros(2, n, nz.ROWS, 2, dtype=torch.int64, device=frames.device)          # by class: a class's frames are 512 cells apart, as the entry adds them
    step = max(c, 1)
    for i, p in enumerate(tab.planes if n else ()):
        head = (p.row_bytes // (tab.sample * step), step) + (() if tab.sample == 1 else (side.depth,))
        _entry_call("savsr_video_noise_stats_u8" if tab.sample == 1 else "savsr_video_noise_stats_u16", frames, n, tab, p, head,
                    (int(bool(interlaced)), out[min(i, 1)].data_ptr()))
    return out.permute(1, 0, 2, 3)


def noise_stats(frames: torch.Tensor, pixel_format: str = "rgb", size=None, depth: int = 8, interlaced: bool = False) -> torch.Tensor:
    """The noise estimator's statistics: int64 [N, 2, 256, 2] on the GPU (savsr_amd.noise.noise_stats_frames is the specification, bit
    for bit), on the caller's current stream, without a sync.  Every 8 x 8 cell of the absolute 3 x 3 second difference
    [1 -2 1]^T (x) [1 -2 1] of a plane adds, with its sum S in 8-bit code units, [n, k, min(S >> 4, 254)] += (1, S), or, where one of its
    rows or columns sums to 0, [n, k, 255, 0] += 1 (a flat cell); field by field with interlaced=True.  Class 0: the Y plane of planar
    frames, or every channel of [N, h, w, c] uint8 frames; class 1: Cb + Cr, zeros where there is none.  Float frames are refused."""
    frames, side, size = _stage_args(frames, pixel_format, size, depth, _noise_frames)
    return _noise_stats_device(frames, side, size, interlaced)


def _estimate_noise_device(frames: torch.Tensor, side: Side, size: Size, interlaced: bool = False, quantile=nz.DEFAULT_QUANTILE,
                           min_cells: int = nz.DEFAULT_MIN_CELLS, floor=nz.DEFAULT_FLOOR) -> "nz.NoiseVerdict":
    """noise.verdict_from_stats on `_noise_stats_device` of frames of the input side on the GPU, summed over the frames there: one device
    -> host copy of 1024 integers."""
    table = _noise_stats_device(frames, side, size, interlaced).sum(0).cpu().numpy()
    return nz.verdict_from_stats(table, quantile, min_cells, floor)


def estimate_noise(frames: torch.Tensor, pixel_format: str = "rgb", size=None, depth: int = 8, interlaced: bool = False,
                   quantile=nz.DEFAULT_QUANTILE, min_cells: int = nz.DEFAULT_MIN_CELLS, floor=nz.DEFAULT_FLOOR) -> "nz.NoiseVerdict":
    """The noise level of a video, from its content: a savsr_amd.noise.NoiseVerdict with sigma and chroma_sigma as exact fractions in
    8-bit code units (None where fewer than `min_cells` cells are not flat, or where there is no chroma); `verdict.spatial_kwargs()` and
    `verdict.denoise_kwargs()` are the explicit arguments of upscale_video beside spatial_denoise= / denoise= that say the same, {} where
    sigma is unknown or below `floor`.  `noise_stats` on the GPU summed over the frames, one host synchronisation, then
    savsr_amd.noise.verdict_from_stats in exact arithmetic: the mean of the quietest `quantile` of the cells, scaled by the constant
    that maps it to sigma for white Gaussian noise.  interlaced=True measures field by field.  The measure, its constants and the gains
    of the two maps are this project's own and are not validated on footage or on trained weights; one figure per video; coarse grain,
    the noise of subsampled chroma and clipped shadows read low, texture over three quarters of the frame reads high."""
    quantile, min_cells, floor = nz.check_quantile(quantile), nz.check_min_cells(min_cells), nz.check_floor(floor)
    frames, side, size = _stage_args(frames, pixel_format, size, depth, _noise_frames)
    return _estimate_noise_device(frames, side, size, interlaced, quantile, min_cells, floor)


# ---- telecined film (savsr_amd/pulldown.py is the specification) -----------------------------------------------------------------------------
def _check_pulldown(pulldown, cycle, fields) -> Optional[str]:
    """pulldown is None or a field order; pulldown_cycle goes with it, and fields= does not."""
    if pulldown is None:
        if isinstance(cycle, bool) or cycle != pd.DEFAULT_CYCLE:
            raise ValueError(f"pulldown_cycle = {cycle!r} goes with pulldown=: it is the decimation cycle of the pulldown removal")
        return None
    check_order(pulldown, "pulldown")
    if fields is not None:
        raise ValueError(f"pulldown = {pulldown!r} together with fields = {fields!r}: they are two answers to one question (telecined film, "
                         f"whose frames are recovered, or interlaced video, whose fields are interpolated); give one of them")
    pd.check_cycle(cycle, "pulldown_cycle")
    return pulldown


def _cells(frames: torch.Tensor, lo: int, hi: int, columns: int) -> torch.Tensor:
    """The output of a reducing entry: int64 [hi - lo, columns] on the frames' device."""
    return torch.empty(max(hi - lo, 0), columns, dtype=torch.int64, device=frames.device)


def _field_scores_device(frames: torch.Tensor, order: str, side: Side, size: Size, lo: int = 0, hi: Optional[int] = None) -> torch.Tensor:
    """savsr_video_field_scores_* on resident frames of the input side on the GPU: int64 [hi - lo, 2] there for source frames [lo, hi)
    (default: all), the previous frame taken among the resident ones and clamped there; enqueued on the current stream (no sync).  Every
    byte of packed frames, the Y plane of planar ones."""
    frames, n, hi, c, tab, oid = _field_job(frames, order, side, size, hi)
    out = _cells(frames, lo, hi, 2)
    if hi > lo:
        _matrix_call("field_scores", frames, n, tab, tab.planes[0], side, (oid, lo, hi, out.data_ptr()))
    return out


def _weave_device(frames: torch.Tensor, order: str, delta: torch.Tensor, side: Side, size: Size, lo: int = 0, hi: Optional[int] = None) -> torch.Tensor:
    """savsr_video_weave on resident frames of the input side on the GPU: the hi - lo woven frames of source frames [lo, hi) (default:
    all) with the device table delta (int32 [hi - lo], -1 | 0).  One call per plane, on the current stream; a byte copy at every depth,
    so one entry with the head of a `_u8` one."""
    frames, n, hi, c, tab, oid = _field_job(frames, order, side, size, hi)
    out = frames.new_empty((max(hi - lo, 0),) + tuple(frames.shape[1:]))
    if hi <= lo:
        return out
    _check_table(delta, "delta", hi - lo, frames.device)
    for p in tab.planes:
        _entry_call("savsr_video_weave", frames, n, tab, p, (p.row_bytes,), (oid, lo, hi, delta.data_ptr(), out.data_ptr(), tab.stride, p.offset))
    return out


def _comb_windows_device(frames: torch.Tensor, order: str, side: Side, size: Size, threshold: int = pd.DEFAULT_COMB_THRESHOLD, lo: int = 0,
                         hi: Optional[int] = None) -> torch.Tensor:
    """savsr_video_comb_windows_* on resident frames of the input side on the GPU: int64 [hi - lo, 2] there for frames [lo, hi) (default:
    all): the largest window count and the total of combed samples; enqueued on the current stream (no sync).  Every byte of packed
    frames with their channel count as the pixel step, the Y plane of planar ones."""
    frames, n, hi, c, tab, oid = _field_job(frames, order, side, size, hi)
    out = _cells(frames, lo, hi, 2)
    if hi > lo:
        _matrix_call("comb_windows", frames, n, tab, tab.planes[0], side, (oid, lo, hi, threshold, out.data_ptr()), max(c, 1))
    return out


def _deinterlace_masked_device(frames: torch.Tensor, order: str, flags: torch.Tensor, method: str, side: Side, size: Size, lo: int = 0,
                               hi: Optional[int] = None) -> torch.Tensor:
    """savsr_video_deinterlace_masked_* on resident frames of the input side on the GPU: hi - lo frames, frame n - lo the same-rate
    deinterlaced frame n where the device table flags (int32 [hi - lo]) is not 0 and a copy of frame n elsewhere; prev / next among the
    resident frames and clamped there.  One call per plane, on the current stream."""
    mid = DEINTERLACERS.index(method)
    frames, n, hi, c, tab, oid = _field_job(frames, order, side, size, hi)
    out = frames.new_empty((max(hi - lo, 0),) + tuple(frames.shape[1:]))
    if hi <= lo:
        return out
    _check_table(flags, "flags", hi - lo, frames.device)
    for p in tab.planes:
        _matrix_call("deinterlace_masked", frames, n, tab, p, side, (oid, lo, hi, out.data_ptr(), tab.stride, p.offset, mid, flags.data_ptr()), max(c, 1))
    return out


def _comb_step(frames: torch.Tensor, side: Side, size: Size) -> int:
    """The samples of a pixel in the matrix the comb measure reads: the channels of packed frames, 1 for planar ones."""
    return max(_field_frames(frames, side, size)[1], 1)


def _clean_combed_device(frames: torch.Tensor, order: str, method: str, threshold: int, pixels: int, side: Side, size: Size, lo: int = 0,
                         hi: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """pulldown.clean_combed on resident woven frames on the GPU, frames [lo, hi): (the cleaned frames, their comb table int64 [hi - lo, 2]
    on the device).  The flags never leave the device: no sync."""
    win = _comb_windows_device(frames, order, side, size, threshold, lo, hi)
    flags = (win[:, 0] >= pixels * _comb_step(frames, side, size)).to(torch.int32).contiguous()
    return _deinterlace_masked_device(frames, order, flags, method, side, size, lo, hi), win


def comb_windows(frames: torch.Tensor, order: str, pixel_format: str = "rgb", size=None, depth: int = 8,
                 threshold: int = pd.DEFAULT_COMB_THRESHOLD) -> torch.Tensor:
    """The residual-comb measure behind combed=: int64 [N, 2] on the GPU (savsr_amd.pulldown.frame_comb_windows is the specification, bit
    for bit), on the caller's current stream, without a sync.  Entry [n, 0] is the largest number of combed samples in any 16-row x
    16-pixel window of frame n (one window every 8 rows and 8 pixels), [n, 1] the number in the whole frame; a sample on a second-field
    row (the rows of the other parity than `order`'s first field) is combed iff |a - b| + |c - b| - |a - c| > 2 * threshold with its
    vertical neighbours a, c.  frames as for `field_scores`.  The default threshold is ffmpeg fieldmatch's cthresh; it is not validated
    on footage."""
    check_order(order)
    pd.check_comb_threshold(threshold, "threshold")
    frames, side, size = _stage_args(frames, pixel_format, size, depth, _field_frames)
    return _comb_windows_device(frames, order, side, size, threshold)


def field_scores(frames: torch.Tensor, order: str, pixel_format: str = "rgb", size=None, depth: int = 8) -> torch.Tensor:
    """The field matcher's scores: int64 [N, 2] on the GPU (savsr_amd.pulldown.frame_scores is the specification, bit for bit), on the
    caller's current stream, without a sync.  Entry [n, j] is the comb measure of frame n with its second field (the rows of the other
    parity than `order`'s first field) taken from frame max(n - 1, 0) (j = 0) or from itself (j = 1).  frames as for `deinterlace`:
    [N, h, w, c] uint8 (every byte), or planar frames with pixel_format=, size=(h, w) (the Y plane; at depth 10 / 12 a sample's 8 most
    significant bits).  Float frames are refused."""
    check_order(order)
    frames, side, size = _stage_args(frames, pixel_format, size, depth, _field_frames)
    return _field_scores_device(frames, order, side, size)


def _delta_device(matches: List[int], device: torch.device) -> torch.Tensor:
    from ._xfer import h2d
    return h2d(torch.tensor(matches, dtype=torch.int32), device)


def _remove_pulldown_device(frames: torch.Tensor, order: str, side: Side, size: Size, cycle: int, combed: Optional[str] = None,
                            comb_threshold: int = pd.DEFAULT_COMB_THRESHOLD, comb_pixels: int = pd.DEFAULT_COMB_PIXELS):
    """pulldown.remove_pulldown_frames on frames of the input side on the GPU: (the kept woven frames, info).  Two host synchronisations:
    the scores come down for the match, the woven frames' pair SADs for the decimation.  combed: the woven frames `comb_windows` flags
    are deinterlaced between the two (the flags stay on the device; the comb table comes down with the SADs)."""
    n = _field_frames(frames, side, size)[0]
    if n < 1:
        raise ValueError("the video has no frames")
    scores = _field_scores_device(frames, order, side, size).cpu()
    matches = pd.matches_from_scores(scores.numpy())
    woven = _weave_device(frames, order, _delta_device(matches, frames.device), side, size)
    extra = {}
    if combed is None:
        sad = [-1] + _pair_sad_device(woven, side, size).cpu().tolist()
    else:
        woven, win = _clean_combed_device(woven, order, combed, comb_threshold, comb_pixels, side, size)
        both = torch.cat([_pair_sad_device(woven, side, size), win.reshape(-1)]).cpu()
        sad, win = [-1] + both[:n - 1].tolist(), both[n - 1:].reshape(n, 2).numpy()
        extra = {"comb": win, "combed": [k for k, f in enumerate(pd.combed_from_windows(win, _comb_step(frames, side, size), comb_pixels)) if f]}
    kept = pd.kept_from_drops(n, pd.drops_from_sad(sad, cycle))
    out = woven.index_select(0, torch.tensor(kept, dtype=torch.int64).to(woven.device))
    return out, {"scores": scores.numpy(), "matches": matches, "sad": torch.tensor(sad, dtype=torch.int64).numpy(), "kept": kept, **extra}


def remove_pulldown(frames: torch.Tensor, order: str, pixel_format: str = "rgb", size=None, depth: int = 8, cycle: int = 5, return_info: bool = False,
                    *, combed: Optional[str] = None, comb_threshold: int = pd.DEFAULT_COMB_THRESHOLD, comb_pixels: int = pd.DEFAULT_COMB_PIXELS):
    """Telecined film (3:2 pulldown) as its film frames: N - N // cycle frames on the GPU in the format of the N given ones
    (savsr_amd.pulldown.remove_pulldown_frames is the specification, bit for bit).  Every frame keeps its first field (order "tff": the
    top rows) and takes the second one from itself or from the frame before it, whichever combs less (`field_scores`); of every `cycle`
    woven frames the one closest to its predecessor (`pair_sad`) is dropped.  frames as for `deinterlace`.  return_info=True: (frames,
    info), info = {"scores", "matches", "sad", "kept"} as in the specification.  Two host synchronisations per call.
    combed="yadif" / "bwdif" (keyword only; hybrid film and video): a woven frame in which some 16 x 16 window still holds comb_pixels
    combed pixels (`comb_windows` with comb_threshold) -- a video insert, a leading frame whose partner field was cut off, the orphan
    field of a broken cadence -- is deinterlaced at same rate by that method, its neighbours being the woven frames; the others pass
    as they are, and the decimation reads the cleaned frames.  info gains "comb" (int64 [N, 2]) and "combed" (the flagged woven
    indices).  The defaults are ffmpeg fieldmatch's (cthresh 9, combpel 80 / 256 of a window's 128 second-field pixels) and are not
    validated on footage; still two host synchronisations."""
    check_order(order)
    cycle = pd.check_cycle(cycle)
    pd.check_comb_options(combed, comb_threshold, comb_pixels, True)
    frames, side, size = _stage_args(frames, pixel_format, size, depth, _field_frames)
    out, info = _remove_pulldown_device(frames, order, side, size, cycle, combed, comb_threshold, comb_pixels)
    return (out, info) if return_info else out


class PulldownRemover:
    """The streaming pulldown removal behind VideoUpscaler(pulldown=...): push(source frames on the GPU) returns the film frames that are
    final, finish() the partial last cycle whole (None if there is none).  The match is causal, so a pushed frame is woven at once, with
    the previous push's last source frame as its context; woven frames wait until their cycle of `cycle` is complete, then the kept ones
    go on.  Between pushes the device keeps one source frame, at most cycle - 1 woven frames and the last woven frame (the next SAD's
    predecessor): `held` <= cycle + 1, copies of their own, so that the chunk they came with is released.  Concatenated, the outputs are
    `remove_pulldown` on the whole video for any chunking; `info` has the matches and the kept indices so far.
    combed="yadif" / "bwdif": as in `remove_pulldown`.  A flagged woven frame is deinterlaced from the woven frames beside it, so a woven
    frame is final (cleaned, or passed as it is) once the next one exists: the last woven frame is held back until the next push, or
    finish(), and the one before it stays as its context; the decimation and the waiting cycle hold cleaned frames.  `held` <= cycle + 3:
    two frames more (one look-ahead, one context).  `info` gains "combed", the flagged woven indices so far."""

    def __init__(self, order: str, side: Side, size: Size, cycle: int = 5, combed: Optional[str] = None,
                 comb_threshold: int = pd.DEFAULT_COMB_THRESHOLD, comb_pixels: int = pd.DEFAULT_COMB_PIXELS):
        check_order(order, "pulldown")
        self.order, self.side, self.size, self.cycle = order, side, size, pd.check_cycle(cycle, "pulldown_cycle")
        self.combed = pd.check_comb_options(combed, comb_threshold, comb_pixels, True)
        self.comb_threshold, self.comb_pixels = comb_threshold, comb_pixels
        self._ctx: Optional[torch.Tensor] = None           # the last source frame pushed
        self._last: Optional[torch.Tensor] = None          # the last woven (combed=: cleaned) frame
        self._pend: Optional[torch.Tensor] = None          # the woven (cleaned) frames of the incomplete cycle, frames [_base, _base + len)
        self._pend_sad: List[int] = []                     # their pair SADs with their predecessors
        self._win = _LookAhead()                           # combed=: the woven context frame, then the woven frames not cleaned yet
        self._cleaned = 0                                  # woven frames that went through the cleaning
        self._base = 0
        self.seen = 0
        self.matches: List[int] = []
        self.kept: List[int] = []
        self.flagged: List[int] = []

    @property
    def held(self) -> int:
        """Frames on the device between pushes: at most cycle + 1, cycle + 3 with combed=."""
        return sum(0 if t is None else int(t.shape[0]) for t in (self._ctx, self._last, self._pend, self._wov))

    @property
    def _wov(self) -> Optional[torch.Tensor]:
        return self._win.buf

    @property
    def info(self) -> dict:
        info = {"matches": list(self.matches), "kept": list(self.kept)}
        if self.combed is not None:
            info["combed"] = list(self.flagged)
        return info

    def push(self, frames: torch.Tensor) -> torch.Tensor:
        k = int(frames.shape[0])
        if k == 0:
            return frames
        src = frames.contiguous() if self._ctx is None else torch.cat([self._ctx, frames], 0)
        n = int(src.shape[0])
        matches = pd.matches_from_scores(_field_scores_device(src, self.order, self.side, self.size, n - k, n).cpu().numpy())
        woven = _weave_device(src, self.order, _delta_device(matches, src.device), self.side, self.size, n - k, n)
        self.matches += matches
        self.seen += k
        self._ctx = src[n - 1:].clone()
        if self.combed is None:
            return self._decimate(woven, None)
        return self._decimate(*self._clean(woven, False))

    def _clean(self, woven: Optional[torch.Tensor], last: bool) -> Tuple[torch.Tensor, torch.Tensor]:
        """The woven frames that are final now, cleaned, and their comb table on the device: all but the newest one, whose next frame is
        not known yet (last: all, the newest one's next frame clamped, as at the end of the video)."""
        buf, lo, hi = self._win.take(woven, last)
        return _clean_combed_device(buf, self.order, self.combed, self.comb_threshold, self.comb_pixels, self.side, self.size, lo, hi)

    def _decimate(self, woven: torch.Tensor, win: Optional[torch.Tensor]) -> torch.Tensor:
        """The next woven (cleaned) frames -> the kept ones of the cycles they complete; the others wait."""
        k = int(woven.shape[0])
        if k == 0:
            return woven
        pairs = woven if self._last is None else torch.cat([self._last, woven], 0)
        sad = _pair_sad_device(pairs, self.side, self.size)
        if win is None:
            sad = sad.cpu().tolist()
        else:          # (the comb table comes down with the SADs: one synchronisation)
            both = torch.cat([sad, win.reshape(-1)]).cpu()
            ns = int(sad.shape[0])
            sad, flags = both[:ns].tolist(), pd.combed_from_windows(both[ns:].numpy(), _comb_step(woven, self.side, self.size), self.comb_pixels)
            self.flagged += [self._cleaned + j for j, f in enumerate(flags) if f]
            self._cleaned += k
        self._pend_sad += ([-1] if self._last is None else []) + sad
        pend = woven if self._pend is None else torch.cat([self._pend, woven], 0)
        full = (int(pend.shape[0]) // self.cycle) * self.cycle
        drops = set(pd.drops_from_sad(self._pend_sad[:full], self.cycle, self._base))
        kept = [j for j in range(self._base, self._base + full) if j not in drops]
        out = pend.index_select(0, torch.tensor([j - self._base for j in kept], dtype=torch.int64).to(pend.device))
        self.kept += kept
        self._pend = pend[full:].clone() if full < int(pend.shape[0]) else None
        self._pend_sad = self._pend_sad[full:]
        self._base += full
        self._last = woven[k - 1:].clone()
        return out

    def finish(self) -> Optional[torch.Tensor]:
        head = None
        if self.combed is not None and self._win.todo:          # the held woven frame, then the end as ever
            head = self._decimate(*self._clean(None, True))
        pend, self._pend, self._ctx, self._last, self._win = self._pend, None, None, None, _LookAhead()
        if pend is None:
            return head if head is not None and int(head.shape[0]) else None
        self.kept += list(range(self._base, self._base + int(pend.shape[0])))
        self._base += int(pend.shape[0])
        self._pend_sad = []
        return pend if head is None else torch.cat([head, pend], 0)


# ---- scan detection (savsr_amd/scan.py is the specification) -----------------------------------------------------------------------------------
def _field_stats_device(frames: torch.Tensor, side: Side, size: Size, lo: int = 0, hi: Optional[int] = None) -> torch.Tensor:
    """savsr_video_field_stats_* on resident frames of the input side on the GPU: int64 [hi - lo, 8] there for source frames [lo, hi)
    (default: all), the previous and the next frame taken among the resident ones and clamped there; one memset and one launch on the
    current stream (no sync).  Every byte of packed frames, the Y plane of planar ones."""
    frames, n, hi, c, tab, _ = _field_job(frames, None, side, size, hi)
    out = _cells(frames, lo, hi, sc.STAT_COLUMNS)
    if hi > lo:
        _matrix_call("field_stats", frames, n, tab, tab.planes[0], side, (lo, hi, out.data_ptr()))
    return out


def field_stats(frames: torch.Tensor, pixel_format: str = "rgb", size=None, depth: int = 8) -> torch.Tensor:
    """The scan detector's statistics: int64 [N, 8] on the GPU (savsr_amd.scan.frame_stats is the specification, bit for bit), on the
    caller's current stream, without a sync.  Row n: the comb measure of frame n with the rows of parity q taken from the previous frame
    (columns 0, 1 for q = 0, 1), from the next frame (2, 3) and from itself (4, 5), the neighbours clamped at the ends of the video, and
    the SAD of field q against the previous frame's (6, 7).  frames as for `field_scores`: [N, h, w, c] uint8 (every byte), or planar
    frames with pixel_format=, size=(h, w) (the Y plane; at depth 10 / 12 a sample's 8 most significant bits).  Float frames and frames
    of one row are refused."""
    frames, side, size = _stage_args(frames, pixel_format, size, depth, _field_frames)
    return _field_stats_device(frames, side, size)


def _detect_scan_device(frames: torch.Tensor, side: Side, size: Size, interlace_threshold=sc.DEFAULT_INTERLACE,
                        progressive_threshold=sc.DEFAULT_PROGRESSIVE, repeat_threshold=sc.DEFAULT_REPEAT) -> "sc.ScanVerdict":
    """scan.verdict_from_stats on `_field_stats_device` of frames of the input side on the GPU: one device -> host copy of 8 N integers."""
    n = _field_frames(frames, side, size)[0]
    stats = _field_stats_device(frames, side, size).cpu().numpy() if n else torch.zeros(0, sc.STAT_COLUMNS, dtype=torch.int64).numpy()
    return sc.verdict_from_stats(stats, interlace_threshold, progressive_threshold, repeat_threshold)


def detect_scan(frames: torch.Tensor, pixel_format: str = "rgb", size=None, depth: int = 8, interlace_threshold=sc.DEFAULT_INTERLACE,
                progressive_threshold=sc.DEFAULT_PROGRESSIVE, repeat_threshold=sc.DEFAULT_REPEAT) -> "sc.ScanVerdict":
    """What kind of scan a video has, from its content: a savsr_amd.scan.ScanVerdict with scan = "progressive", "interlaced", "telecine"
    or "undetermined" and order = "tff" / "bff" / None; `verdict.kwargs()` is the explicit argument of upscale_video / VideoUpscaler
    that says the same ({"fields": order}, {"pulldown": order} or {}).  `field_stats` on the GPU, one host synchronisation, then
    savsr_amd.scan.verdict_from_stats in exact arithmetic: the 3:2 cadence of repeated fields first, then whether a frame's two fields
    fit each other better than the neighbouring frames' (progressive), then which field order makes the temporal neighbours fit
    (interlaced).  Static or flat video is undetermined.  The rule and its thresholds are this project's own (ffmpeg idet is the idea)
    and are not validated on real footage; one verdict per video: mixed content, 2:2 PAL film, cadences other than 3:2 and fades are
    not handled.  frames as for `field_stats`."""
    sc.check_thresholds(interlace_threshold, progressive_threshold, repeat_threshold)
    frames, side, size = _stage_args(frames, pixel_format, size, depth, _field_frames)
    return _detect_scan_device(frames, side, size, interlace_threshold, progressive_threshold, repeat_threshold)


class ScanStats:
    """The streaming form of `field_stats`, beside FieldSplitter: push(source frames on the GPU) returns the rows that are final (int64
    [k, 8] on the GPU), finish() the last frame's row (None without a pushed frame).  A frame's row needs the frame after it, so the
    last pushed frame is held back; with the frame before it (the context) the device keeps at most two source frames between pushes
    (copies of their own, so that the chunk they came with is released).  Concatenated, the rows are `field_stats` on the whole video
    for any chunking.  stats: the function of (frames, side, size, lo, hi) that computes rows (the kernel's wrapper)."""

    def __init__(self, side: Side, size: Size, stats=None):
        self.side, self.size = side, size
        self._stats = _field_stats_device if stats is None else stats
        self._win = _LookAhead()                          # source frames [seen - held, seen)
        self.seen = 0

    @property
    def _src(self) -> Optional[torch.Tensor]:
        return self._win.buf

    @property
    def held(self) -> int:
        """Source frames on the device between pushes: at most two."""
        return self._win.held

    def push(self, frames: torch.Tensor) -> torch.Tensor:
        self.seen += int(frames.shape[0])
        src, lo, hi = self._win.take(frames)
        return self._stats(src, self.side, self.size, lo, hi)

    def finish(self) -> Optional[torch.Tensor]:
        src, lo, hi = self._win.take(None, True)
        if hi <= lo:          # nothing was pushed (or finish() ran before)
            return None
        return self._stats(src, self.side, self.size, lo, hi)


def _check_scan(scan, fields, pulldown, pulldown_cycle, auto_ok: bool = True) -> Optional[str]:
    """scan is None or "detect"; "detect" excludes fields=, pulldown= and a pulldown_cycle other than 5."""
    if sc.check_scan(scan) is None:
        return None
    if not auto_ok:
        raise ValueError("scan = 'detect' in VideoUpscaler: the decision needs the video; run savsr_amd.detect_scan on a probe chunk "
                         "first and give its answer as fields= or pulldown= (verdict.kwargs()), or use python -m savsr_amd.upscale --scan detect")
    if fields is not None or pulldown is not None:
        given = f"fields = {fields!r}" if fields is not None else f"pulldown = {pulldown!r}"
        raise ValueError(f"scan = 'detect' together with {given}: the detector answers the question that argument answers; give one of them")
    if isinstance(pulldown_cycle, bool) or pulldown_cycle != pd.DEFAULT_CYCLE:
        raise ValueError(f"scan = 'detect' with pulldown_cycle = {pulldown_cycle!r}: the detector knows the 3:2 cadence only (cycle "
                         f"{pd.DEFAULT_CYCLE}); give pulldown= with that cycle")
    return scan


def _check_field_options(deinterlacer, field_rate, fields, pulldown, detect: bool = False) -> None:
    """deinterlacer= / field_rate= say how fields= (or an interlaced verdict of scan="detect") is carried out: refused by name when
    unknown, without either when not at their defaults, and together with pulldown=."""
    check_method(deinterlacer, "deinterlacer")
    check_rate(field_rate, "field_rate")
    for name, value, default in (("deinterlacer", deinterlacer, DEINTERLACERS[0]), ("field_rate", field_rate, FIELD_RATES[0])):
        if value == default:
            continue
        if pulldown is not None:
            raise ValueError(f"{name} = {value!r} together with pulldown = {pulldown!r}: the pulldown removal weaves fields and interpolates "
                             f"nothing; {name} goes with fields=")
        if fields is None and not detect:
            raise ValueError(f"{name} = {value!r} goes with fields=: without interlaced video there are no fields to interpolate")


def make_stage(fields, pulldown, pulldown_cycle, side: Side, size: Size, deinterlacer: str = "yadif", field_rate: str = "double", combed=None,
               comb_threshold: int = pd.DEFAULT_COMB_THRESHOLD, comb_pixels: int = pd.DEFAULT_COMB_PIXELS):
    """The streaming stage in front of everything else that fields= / pulldown= / pulldown_cycle= ask for, on frames of `side`: None, a
    FieldSplitter or a PulldownRemover (the two exclude each other), after `_check_fields`, `_check_pulldown`,
    `_check_field_options` (deinterlacer= / field_rate=, which the FieldSplitter takes) and `pulldown.check_comb_options` (combed= /
    comb_threshold= / comb_pixels=, which the PulldownRemover takes), in that order."""
    _check_fields(fields)
    _check_pulldown(pulldown, pulldown_cycle, fields)
    _check_field_options(deinterlacer, field_rate, fields, pulldown)
    pd.check_comb_options(combed, comb_threshold, comb_pixels, pulldown is not None, fields)
    if fields is not None:
        return FieldSplitter(fields, side, size, deinterlacer, field_rate)
    return None if pulldown is None else PulldownRemover(pulldown, side, size, pulldown_cycle, combed, comb_threshold, comb_pixels)
