"""Whole LR videos in, SR videos out: the sequence path behind `SAVSR.upscale_video` and `VideoUpscaler`.

Output frame i is what the reference pipeline gives for it: the frame's window by generate_frame_indices with the chosen padding
(lbasicsr/data/data_util.py:63-112, `harness.window_indices`), then SAVSR.forward on that window; with out="uint8", tensor2img's
clamp / x255 / round half to even (lbasicsr/utils/img_util.py:66-90) without the BGR swap.  The frames stay on the device: the
windows are gathered there and the result is quantised there, by one path for every kind of frame, HipEngine.forward_video.

Three modules, one above the other.  savsr_amd/frames.py names the frames: the formats, the argument checks, the plane table, and
`VideoSpec` -- what the frames on either side of the network are (pixel_format / out, size, depth / out_depth, colour / out_colour,
siting / out_siting, chroma_filter, num_in_ch) as one value, checked once, in a fixed order, by `video_spec`; everything behind it
(upscale_video, VideoUpscaler, the cut detector, the engine) reads the spec and checks nothing again.  It holds names only; the integer
ids of the C ABI are computed beside the calls that take them.  savsr_amd/prepass.py is everything that runs on the device in front of
the network.  This module runs the windows: `upscale_video`, `VideoUpscaler`, `window_lists`; the public names of the other two are
importable from here as they always were.  SAVSR.upscale_video documents every argument; what the sequence path makes of them:

cuts=[k, ...] / cuts="auto": the video is a sequence of scenes and every scene is treated as a video of its own (savsr_amd/scenes.py:
windows stop at cuts); "auto" finds the cuts on the device (savsr_video_pair_sad_*, then scdet's rule on the host).

fields= / pulldown= (one of them), then crop=: stages in front of everything else, in that order, so the call is, bit for bit, the call
on `deinterlace(frames, fields, ...)` (2N progressive frames), on `remove_pulldown(frames, pulldown, ...)` (the N - N // pulldown_cycle
film frames), on the hand-cropped video (crop="auto" finds the rect on the device; bars="keep" puts the result back into full-size
frames of nominal black, bars="drop" returns the picture alone; both are strided copies through torch views).  Each argument at None
runs exactly the lines that ran before it existed.  combed= / comb_threshold= / comb_pixels= belong to pulldown= (savsr_amd/pulldown.py:
woven frames that are still combed are deinterlaced before the decimation) and are `remove_pulldown`'s arguments of the same names.

scan="detect": the call finds out which of the two the video is (savsr_amd/scan.py: `detect_scan` on the unpacked frames on the device,
right after surface= unpacking and in front of everything else) and continues exactly as if the verdict's `kwargs()` had been given:
fields=order for interlaced video, pulldown=order for telecined film, nothing for progressive and undetermined video.

denoise="ata": temporal noise reduction (savsr_amd/denoise.py: ffmpeg atadenoise's serial rule, two independent walks over the frames
before and after) behind surface= unpacking, scan="detect" and fields= / pulldown= -- it needs progressive frames -- and in front of the
crop, the cuts and the windows: the call is, bit for bit, the call on `denoise_video(v', ...)`, v' the deinterlaced or pulldown-removed
video.  The rule is per sample, so it commutes with crop= exactly; cuts="auto" scores the denoised frames.  None runs the lines that ran
before.

spatial_denoise="nlm": spatial noise reduction (savsr_amd/nlmeans.py: non-local means in integers, every frame on its own) behind
denoise= and behind the crop, in front of the cuts and the windows.  The rule does not commute with a crop, so the place is part of the
contract: with crop=None the call is, bit for bit, the call on `denoise_spatial(v', ...)`, v' the video after fields= / pulldown= /
denoise=; with crop=rect and bars="drop" it is the call on `denoise_spatial(crop_frames(v', rect), ...)`, and with bars="keep" the
picture inside the bars is those bytes.  cuts="auto" scores the filtered frames; crop="auto" still reads the unfiltered ones.  None runs
the lines that ran before.

deblock="weak" / "strong": deblocking (savsr_amd/deblock.py: a filter across the edges of a fixed block grid, pass X then pass Y, every
frame on its own).  The grid belongs to the coded frame, so the stage runs on the frames as decoded: right after surface= unpacking and
after scan="detect" has read the unfiltered frames, in front of fields= / pulldown=, denoise=, the crop, spatial_denoise= and the cuts, and
field by field exactly when the video is treated as interlaced (fields= or pulldown= given, or an interlaced / telecine verdict).  The
call is, bit for bit, the call on `deblock_video(v, ..., interlaced=I)`; crop= crops the filtered frames, so crop="auto" reads filtered
frames.  None runs the lines that ran before.  deblock_origin=(oy, ox) / deblock_chroma_origin= say where the grid's first edges lie
(a video cropped by c samples before it arrived has them at (-c) mod block; the chroma planes of 4:2:0 / 4:2:2 frames have an origin of
their own, in chroma samples, which must be named beside a luma origin other than (0, 0)).  deblock_grid="auto" asks the frames instead
(savsr_amd/grid.py: `grid_stats` on the frames the deblocker will read -- after surface= unpacking and after scan="detect", field-wise
exactly when the deblocker runs field-wise -- summed over the video, one more host synchronisation, then an exact rule on the host): the
call is, bit for bit, the call with `verdict.kwargs()` given, and with a "no grid" verdict the call with deblock=None; chroma planes whose
grid was not found at the luma's block are left alone (chroma threshold a = 0).  One grid per video; the rule's defaults are this
project's own and are not validated on footage.

dering="cdef": deringing (savsr_amd/dering.py: a direction per 8 x 8 block, a constrained filter along and across it, every frame on its
own).  Ringing belongs to the coded frame as the block grid does, and codecs dering after they deblock: the stage runs right behind
deblock= on the frames as decoded -- after surface= unpacking and after scan="detect" and deblock_grid="auto" have read their frames, in
front of fields= / pulldown=, denoise=, the crop, spatial_denoise= and the cuts -- and field by field exactly when the deblocker would.
The call is, bit for bit, the call on `dering_video(deblock_video(v, ...), ..., interlaced=I)`.  None runs the lines that ran before.

denoise_strength="auto" / spatial_strength="auto" (beside denoise= / spatial_denoise=): the strength from the frames' noise level
(savsr_amd/noise.py: `noise_stats` summed over the video on the GPU, one launch per plane and one host synchronisation each, an exact
rule on the host).  Each is measured on the frames its stage will read: the temporal one right in front of the temporal denoiser (after
surface=, deblock=, dering= and fields= / pulldown=, on progressive frames), the spatial one right in front of the spatial denoiser
(after denoise= and the crop, so it sees the noise that is left).  The call is, bit for bit, the call with `verdict.denoise_kwargs()` /
`verdict.spatial_kwargs()` given, and where no noise is found the call without that stage; an explicit chroma strength beside "auto"
wins over the found one.  One figure per video; the measure, its constants and the gains are this project's own and are not validated
on footage.

dither="ordered": every quantiser behind the network (packed uint8, planar YUV, the luma-only path's Y plane) takes floor(t + theta(y, x))
in rint's place, theta from a 16 x 16 Bayer matrix at the sample's position in its plane (savsr_amd/dither.py is the specification, the
`_d` entries of the C ABI the kernels).  It belongs to the quantiser: bars="keep" inserts exact nominal black after it and out_surface
packs after that.  None runs the quantisers as they were; with out="float" there is nothing to quantise and the argument is refused.

surface= / out_surface=: where the samples of planar frames lie in memory on either side (savsr_amd/surface.py: NV12, P010, UYVY, pitched
planar, ...).  The frames are unpacked right after the host-to-device copy, in front of fields=, pulldown=, crop= and everything else, and
the result is packed last, after the bars are re-inserted: the call is, bit for bit, the call on `unpack_surface(frames, surface, ...)`,
and its result `pack_surface(result, out_surface, ...)` at the output's size and depth.  One launch each; nothing between them changes.

Every argument is checked here, on the host, before anything is enqueued on the GPU.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import torch

from . import active, scenes
from .frames import (OUT_KINDS, PADDING_MODES, PIXEL_FORMATS, SAMPLE_FORMATS, YUV_FORMATS, Side, VideoSpec, as_scale,  # noqa: F401  (re-exported)
                     check_colours, check_depths, check_length, check_out, check_padding, check_pixel_format, check_sample_alignment,
                     check_sitings, chroma_of, frame_layout, i420_layout, layout_of, luma_mode, video_spec)
from .harness import window_indices
from .packing import get_hw
from .deblock import check_deblock_options, check_origins
from .denoise import check_denoise_options
from .dering import check_dering_options
from .nlmeans import check_spatial_options
from .prepass import (FieldSplitter, PulldownRemover, ScanStats, TemporalDenoiser, _check_crop_args, _check_field_options, _check_fields,  # noqa: F401  (re-exported)
                      _check_pulldown, _check_scan, _crop_device, _cropped_spec, _deblock_device, _deinterlace_device, _dering_device, _denoise_device, _denoise_frames, _denoise_spatial_device,
                      _detect_device, _detect_grid_device, _detect_scan_device, _estimate_noise_device, _field_frames, _insert_device, _pair_sad_device, _pack_surface_device,
                      _remove_pulldown_device, _sample_frames, _to_device, _unpack_surface_device, comb_windows, deblock_video, deinterlace, denoise_spatial, denoise_video, dering_video,
                      detect_active_area, detect_cuts, detect_grid, detect_scan, estimate_noise, field_scores, field_stats, grid_stats, line_sums, make_denoiser, make_stage, noise_stats,
                      pack_surface, pair_sad, remove_pulldown, surface_layout, surface_side, surface_table, unpack_surface)
from .pulldown import check_comb_options
from .grid import GridVerdict  # noqa: F401  (re-exported)
from .noise import NoiseVerdict, is_auto as _auto_strength  # noqa: F401  (re-exported)
from .scan import ScanVerdict, check_thresholds  # noqa: F401  (re-exported)


def _check_net(net) -> None:
    if net.training:
        raise RuntimeError("savsr_amd.SAVSR implements the inference path only; call .eval() first")


def _net_device(net) -> torch.device:
    """The GPU the network is on; refuses a network that is not on one."""
    dev = net.gamma.device
    if dev.type != "cuda":
        raise RuntimeError("savsr_amd runs on an AMD GPU only: move the network to the GPU (net.cuda()) first")
    return dev


def _is_auto(cuts) -> bool:
    return isinstance(cuts, str) and cuts == "auto"


def check_cuts_arg(cuts) -> None:
    """cuts is None, "auto" or a sequence of frame indices (the indices themselves: scenes.check_cuts, once the length is known)."""
    if cuts is None or _is_auto(cuts):
        return
    if isinstance(cuts, (str, bytes)):
        raise ValueError(f"cuts = {cuts!r}: None, 'auto' or a sequence of frame indices")
    scenes.check_cuts(cuts, None)


def _out_hw(h: int, w: int, crop, bars: str, sc):
    """The size of the frames a call returns: of the full frame, or of the rect alone with bars="drop"."""
    return get_hw(*((h, w) if crop is None or bars == "keep" else crop[2:]), sc)


def upscale_video(net, frames: torch.Tensor, scale=None, padding: str = "reflection", out: str = "float", pixel_format: str = "rgb",
                  size=None, cuts: Union[None, str, Sequence[int]] = None, scene_threshold=10.0, colour: str = "bt601",
                  out_colour: Optional[str] = None, depth: int = 8, out_depth: Optional[int] = None, siting: Optional[str] = None,
                  out_siting: Optional[str] = None, chroma_filter: Optional[str] = None, crop=None, crop_limit=24,
                  bars: str = "keep", fields: Optional[str] = None, pulldown: Optional[str] = None, pulldown_cycle: int = 5, *,
                  surface=None, out_surface=None, scan: Optional[str] = None, dither: Optional[str] = None, deinterlacer: str = "yadif",
                  field_rate: str = "double", combed: Optional[str] = None, comb_threshold: int = 9, comb_pixels: int = 40,
                  denoise: Optional[str] = None, denoise_radius: int = 4, denoise_strength=(4, 9), denoise_chroma_strength=None,
                  spatial_denoise: Optional[str] = None, spatial_patch: int = 3, spatial_search: int = 7, spatial_strength=3.0,
                  spatial_chroma_strength=None, deblock: Optional[str] = None, deblock_block: int = 8, deblock_strength=(25, 13),
                  deblock_chroma_strength=None, deblock_origin=(0, 0), deblock_chroma_origin=None, deblock_grid: Optional[str] = None,
                  dering: Optional[str] = None, dering_strength=(4, 2), dering_chroma_strength=None, dering_damping: int = 5) -> torch.Tensor:
    """SAVSR.upscale_video (see there)."""
    _check_net(net)
    check_padding(padding)
    spec = video_spec(net.cfg["num_in_ch"], out, pixel_format, size, colour, out_colour, depth, out_depth, siting, out_siting, chroma_filter,
                      dither)
    sc = as_scale(net.scale if scale is None else scale)
    noise = check_denoise_options(denoise, denoise_radius, denoise_strength, denoise_chroma_strength)          # None: the path as it was
    grain = check_spatial_options(spatial_denoise, spatial_patch, spatial_search, spatial_strength, spatial_chroma_strength)          # likewise
    edges = check_deblock_options(deblock, deblock_block, deblock_strength, deblock_chroma_strength, origin=deblock_origin,
                                  chroma_origin=deblock_chroma_origin, grid=deblock_grid)          # likewise
    rings = check_dering_options(dering, dering_strength, dering_chroma_strength, dering_damping)          # likewise
    grid = None          # (origin, chroma origin) of the deblocker's grid, or "auto": found below, on the frames the deblocker will read
    if edges is not None:              # (an odd oy is refused here where the run is known to be field-wise, and below once scan= has said so)
        grid = "auto" if deblock_grid == "auto" else check_origins(deblock_origin, deblock_chroma_origin, edges[0], fields is not None or pulldown
                                                                   is not None, spec.inp.layout, "deblock_")
    if surface is not None:            # the frames lie in a surface: checked against it, unpacked below, and planar from there on
        in_tab = surface_table(surface, spec.inp, spec.size)
        n, (h, w) = surface_layout(frames, in_tab), spec.size
        shaped = torch.empty(min(n, 1), spec.inp.frame_bytes(h, w), dtype=torch.uint8)          # the frames the stages will be given, by shape
        spec.frames_hw(shaped)             # (the network's channels, in the planar path's words)
    else:
        n, h, w = spec.frames_hw(frames)
        shaped = frames
    if out_surface is not None:        # (its table: once the crop is checked, or found)
        surface_side(out_surface, spec.out, "out_surface")
    if edges is not None:              # (integer samples only, and the stage comes first: its refusal of float frames speaks first)
        _sample_frames(shaped, spec.inp, spec.size, "deblock")
    if rings is not None:
        _sample_frames(shaped, spec.inp, spec.size, "dering")
    if noise is not None or grain is not None:          # (integer samples only: float frames are refused here, before the GPU is touched)
        _denoise_frames(shaped, spec.inp, spec.size)
    # (deinterlacer= / field_rate= also go with scan="detect": they say how an interlaced verdict is carried out)
    _check_field_options(deinterlacer, field_rate, fields, pulldown, scan is not None)
    # (combed= also goes with scan="detect": it says how a telecine verdict is carried out, and is ignored for the other verdicts)
    check_comb_options(combed, comb_threshold, comb_pixels, pulldown is not None or scan is not None, fields)
    if _check_scan(scan, fields, pulldown, pulldown_cycle) is not None:          # the content says what fields= / pulldown= would have said
        _field_frames(shaped, spec.inp, spec.size)
        _check_crop_args(crop, crop_limit, bars)          # (what does not depend on the verdict speaks before the GPU is touched)
        check_cuts_arg(cuts)
        frames = _to_device(frames, _net_device(net))
        if surface is not None:            # the surface comes first of all: the detector sees planar frames; unpacked once, here
            frames, surface = _unpack_surface_device(frames, in_tab, spec.inp, spec.size), None
        found = _detect_scan_device(frames, spec.inp, spec.size).kwargs()
        fields, pulldown = found.get("fields"), found.get("pulldown")
        if pulldown is None:
            combed = None
    if _check_fields(fields) is not None:          # everything below sees the progressive video of 2N frames (field_rate "same": N)
        _field_frames(shaped, spec.inp, spec.size)
        if field_rate != "same":
            n *= 2
    if _check_pulldown(pulldown, pulldown_cycle, fields) is not None:          # everything below sees the film of N - N // cycle frames
        _field_frames(shaped, spec.inp, spec.size)
        n -= n // pulldown_cycle
    crop = _check_crop_args(crop, crop_limit, bars)
    if crop is not None and crop != "auto":
        crop = active.check_rect(crop, h, w, spec.inp.layout)
    if out_surface is not None and crop != "auto":
        surface_table(out_surface, spec.out, _out_hw(h, w, crop, bars, sc), "out_surface")
    T = net.num_frame
    if cuts is None:
        check_length(n, T, padding)
    else:
        check_cuts_arg(cuts)
        scenes.check_threshold(scene_threshold)
        if n < 1:
            raise ValueError("the video has no frames")
        if not _is_auto(cuts):
            cuts = scenes.check_cuts(cuts, n)
    frames = _to_device(frames, _net_device(net))
    if surface is not None:            # the surface comes first of all: everything below sees planar frames
        frames = _unpack_surface_device(frames, in_tab, spec.inp, spec.size)
    if edges is not None:              # the block grid belongs to the frames as decoded: field by field where the video is treated as interlaced
        fieldwise = fields is not None or pulldown is not None
        if grid == "auto":             # block and origins from the frames the deblocker will read; no grid: the stage is left out
            edges, grid = _auto_grid(_detect_grid_device(frames, spec.inp, spec.size, fieldwise), edges, fieldwise, spec.inp.layout)
        else:
            grid = check_origins(*grid, edges[0], fieldwise, spec.inp.layout, "deblock_")
        if edges is not None:
            frames = _deblock_device(frames, spec.inp, spec.size, *edges, fieldwise, *grid)
    if rings is not None:              # ringing belongs to the frames as decoded too: right behind the deblocker, field by field when it would be
        frames = _dering_device(frames, spec.inp, spec.size, *rings, fields is not None or pulldown is not None)
    if fields is not None:             # deinterlacing comes first, before the crop
        frames = _deinterlace_device(frames, fields, spec.inp, spec.size, method=deinterlacer, rate=field_rate)
    if pulldown is not None:           # pulldown removal comes first, where deinterlacing comes
        frames = _remove_pulldown_device(frames, pulldown, spec.inp, spec.size, pulldown_cycle, combed, comb_threshold, comb_pixels)[0]
    if noise is not None and noise[1] == "auto":          # the strength from the frames the denoiser will read; no noise: the stage is left out
        noise = _auto_denoise(_estimate_noise_device(frames, spec.inp, spec.size), noise)
    if noise is not None:              # the denoiser sees progressive frames, and the crop, the cuts and the windows see its output
        frames = _denoise_device(frames, spec.inp, spec.size, *noise)
    full = spec
    if crop == "auto":
        crop = _detect_device(frames, spec.inp, spec.size, crop_limit)
    if crop == (0, 0, h, w):          # the whole frame: the uncropped path
        crop = None
    if crop is not None:               # the crop comes first: everything below sees the cropped video
        frames = _crop_device(frames, crop, spec.inp, (h, w))
        spec = _cropped_spec(spec, crop)
    if grain is not None and grain[2] == "auto":          # likewise, on what the temporal denoiser and the crop have left
        grain = _auto_spatial(_estimate_noise_device(frames, spec.inp, spec.size), grain)
    if grain is not None:              # the spatial denoiser sees the cropped picture (the bars never enter a patch); the cuts and the windows see its output
        frames = _denoise_spatial_device(frames, spec.inp, spec.size, *grain)
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
            res = _insert_device(res, active.place(crop, h, w, sc, full.out.layout), full)
        if out_surface is not None:    # the surface comes last of all, after the bars are back
            HW = _out_hw(h, w, crop, bars, sc)
            res = _pack_surface_device(res, surface_table(out_surface, full.out, HW, "out_surface"), full.out, HW)
        return res


def _auto_grid(verdict, edges, fieldwise: bool, layout):
    """What deblock_grid="auto" continues with: ((block, mode, strength, chroma strength), (origin, chroma origin)) as if
    `verdict.kwargs()` had been given beside deblock=, or (None, None) without a grid (the call with deblock=None)."""
    found = verdict.kwargs()
    if not found:
        return None, None
    edges = (found["deblock_block"], edges[1], edges[2], found.get("deblock_chroma_strength", edges[3]))
    return edges, check_origins(found["deblock_origin"], found.get("deblock_chroma_origin"), edges[0], fieldwise, layout, "deblock_")


def _auto_denoise(verdict, noise):
    """What denoise_strength="auto" continues with: (radius, strength, chroma strength) as if `verdict.denoise_kwargs()` had been
    given beside denoise=, an explicit chroma strength before the found one; None where no noise was found (the call with denoise=None)."""
    found = verdict.denoise_kwargs()
    if not found:
        return None
    chroma = found.get("denoise_chroma_strength") if noise[2] is None else noise[2]
    return check_denoise_options("ata", noise[0], found["denoise_strength"], chroma)


def _auto_spatial(verdict, grain):
    """What spatial_strength="auto" continues with: (patch, search, strength, chroma strength) as if `verdict.spatial_kwargs()` had
    been given beside spatial_denoise=, an explicit chroma strength before the found one; None where no noise was found."""
    found = verdict.spatial_kwargs()
    if not found:
        return None
    chroma = found.get("spatial_chroma_strength") if grain[3] is None else grain[3]
    return check_spatial_options("nlm", grain[0], grain[1], found["spatial_strength"], chroma)


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

    Every format argument (pixel_format, size, out, chroma_filter, colour, depth, siting and their out_ forms) is upscale_video's, with
    chunks of [k, yuv.frame_bytes(h, w, depth, chroma)] uint8 for planar frames.

    cuts=[k, ...] (global frame indices) or cuts="auto" (each push scores its new pairs on the device, the pair with the previous
    push's last frame included, and decides with `scene_threshold`): windows stop at cuts as in upscale_video(cuts=...), and `up.cuts`
    lists the cuts among the frames pushed so far.  A frame is returned once its window is the same however the video continues -- a cut
    may still come anywhere after the last pushed frame (savsr_amd.scenes.ScenePlan); the frames kept are bounded as without cuts.

    crop=(y0, x0, ah, aw), bars="keep" / "drop": as in upscale_video, with an explicit rect only ("auto" needs the whole video: detect
    first with savsr_amd.detect_active_area).  Chunks are checked against the full frame size and cropped as they arrive, so the device
    buffer holds cropped frames; `spec` is the VideoSpec of the cropped size.

    fields="tff" / "bff": interlaced chunks, as in upscale_video, through a prepass.FieldSplitter: a source frame becomes two progressive
    frames once the frame after it has been pushed, so push() holds the last source frame back and finish() flushes it (at most two more
    source frames on the device between pushes).  The cuts, the crop and the windows operate on the progressive frames as they are
    produced, and explicit cuts index them.  deinterlacer="bwdif" / field_rate="same" (keyword only): as in upscale_video; the same
    source frame is held back for both, and with "same" a source frame becomes one progressive frame.

    pulldown="tff" / "bff", pulldown_cycle=5: telecined chunks, as in upscale_video, through a prepass.PulldownRemover: a pushed frame is
    woven at once, woven frames wait until their cycle is complete, and finish() flushes the partial last cycle whole (at most
    pulldown_cycle + 1 more frames on the device between pushes; two host synchronisations per push).  `pulldown_info` has the matches
    and the kept indices so far.  combed="yadif" / "bwdif", comb_threshold=9, comb_pixels=40 (keyword only): as in upscale_video; a
    woven frame is final once the next one exists, so the stage holds two frames more (pulldown_cycle + 3), and `pulldown_info` gains
    "combed", the woven frames that were deinterlaced.

    surface= / out_surface= (savsr_amd.surface.Surface): as in upscale_video; every pushed chunk is [k, stride] uint8 in `surface` and is
    unpacked as it arrives, every returned chunk is packed into `out_surface` as it leaves.  The conversion is stateless, so any chunking
    gives the same frames.

    dither= (keyword only): as in upscale_video.  The pattern depends on the sample's position in the frame alone, never on the frame's
    index, so any chunking gives the same frames.

    denoise="ata", denoise_radius=4, denoise_strength=(4, 9), denoise_chroma_strength=None (keyword only): temporal noise reduction, as in
    upscale_video, through a prepass.TemporalDenoiser chained behind the fields= / pulldown= stage: a progressive frame goes on once
    denoise_radius frames after it have arrived, so push() holds that many back and finish() flushes them; the device keeps at most
    2 * denoise_radius more frames between pushes (denoise_radius behind as context, denoise_radius not done yet).  The cuts, the crop
    and the windows operate on the denoised frames; any chunking gives the same frames.

    spatial_denoise="nlm", spatial_patch=3, spatial_search=7, spatial_strength=3.0, spatial_chroma_strength=None (keyword only): spatial
    noise reduction, as in upscale_video.  The stage is stateless -- every frame is filtered on its own -- so it runs on the frames as
    they are cropped and buffered, holds no frame back and keeps none; any chunking gives the same frames.  The default strength is a
    parameter: nothing is validated on footage.

    deblock="weak" / "strong", deblock_block=8, deblock_strength=(25, 13), deblock_chroma_strength=None (keyword only): deblocking, as in
    upscale_video, on every pushed chunk as it arrives (after surface= unpacking, in front of the fields= / pulldown= stage), field by
    field exactly when fields= or pulldown= is given.  The stage is stateless -- every frame is filtered on its own -- so it holds
    nothing back and any chunking gives the same frames.  The defaults are parameters: nothing is validated on footage.
    deblock_origin=(0, 0), deblock_chroma_origin=None: the grid's origin, as in upscale_video.  deblock_grid="auto" is refused: the
    decision needs the video.  Run savsr_amd.detect_grid on a probe chunk (or sum savsr_amd.grid_stats over a first pass, as
    python -m savsr_amd.upscale --deblock-grid auto does) and give `verdict.kwargs()`.

    dering="cdef", dering_strength=(4, 2), dering_chroma_strength=None, dering_damping=5 (keyword only): deringing, as in upscale_video,
    on every pushed chunk right behind the deblocker (in front of the fields= / pulldown= stage), field by field exactly when fields= or
    pulldown= is given.  The stage is stateless -- every frame is filtered on its own -- so it holds nothing back and any chunking
    gives the same frames.  The defaults are parameters: nothing is validated on footage.

    denoise_strength="auto" and spatial_strength="auto" are refused: the decision needs the video.  Run savsr_amd.estimate_noise on a
    probe chunk (or sum savsr_amd.noise_stats over a first pass, as python -m savsr_amd.upscale --denoise-strength auto does) and give
    `verdict.denoise_kwargs()` / `verdict.spatial_kwargs()`.

    scan="detect" is refused: the decision needs the video.  Run savsr_amd.detect_scan on a probe chunk (or prepass.ScanStats over a
    first pass, as python -m savsr_amd.upscale --scan detect does) and give its answer as fields= / pulldown=."""

    def __init__(self, net, scale=None, padding: str = "reflection", out: str = "float", pixel_format: str = "rgb", size=None,
                 cuts: Union[None, str, Sequence[int]] = None, scene_threshold=10.0, colour: str = "bt601", out_colour: Optional[str] = None,
                 depth: int = 8, out_depth: Optional[int] = None, siting: Optional[str] = None, out_siting: Optional[str] = None,
                 chroma_filter: Optional[str] = None, crop=None, bars: str = "keep", fields: Optional[str] = None, pulldown: Optional[str] = None,
                 pulldown_cycle: int = 5, *, surface=None, out_surface=None, scan: Optional[str] = None, dither: Optional[str] = None,
                 deinterlacer: str = "yadif", field_rate: str = "double", combed: Optional[str] = None, comb_threshold: int = 9,
                 comb_pixels: int = 40, denoise: Optional[str] = None, denoise_radius: int = 4, denoise_strength=(4, 9),
                 denoise_chroma_strength=None, spatial_denoise: Optional[str] = None, spatial_patch: int = 3, spatial_search: int = 7,
                 spatial_strength=3.0, spatial_chroma_strength=None, deblock: Optional[str] = None, deblock_block: int = 8,
                 deblock_strength=(25, 13), deblock_chroma_strength=None, deblock_origin=(0, 0), deblock_chroma_origin=None,
                 deblock_grid: Optional[str] = None, dering: Optional[str] = None, dering_strength=(4, 2), dering_chroma_strength=None,
                 dering_damping: int = 5):
        _check_net(net)
        check_padding(padding)
        _check_scan(scan, fields, pulldown, pulldown_cycle, auto_ok=False)          # (None is the only value that passes: the path as it was)
        check_out(out, net.cfg["num_in_ch"], chroma_filter)          # (speaks before the cuts, video_spec after them: the order of refusals)
        self._plan = None                          # scenes.ScenePlan when cuts are given; None: the path without cuts, as it was
        if cuts is not None:
            check_cuts_arg(cuts)
            self._threshold = scenes.check_threshold(scene_threshold)
            self._auto = _is_auto(cuts)
            self._given = [] if self._auto else scenes.check_cuts(cuts, None)       # explicit cuts not reached yet
            self._prev_sad = 0                     # the last pair's score (scdet's damping term), carried from push to push
            self._plan = scenes.ScenePlan(net.num_frame, padding)
        # the frames on both sides, checked once, here; the luma-only path (`luma_mode`) is decided with them
        self.spec = video_spec(net.cfg["num_in_ch"], out, pixel_format, size, colour, out_colour, depth, out_depth, siting, out_siting, chroma_filter,
                               dither)
        self._full = self.spec                     # the spec of the chunks as pushed; `spec` becomes the cropped size's with a crop
        self._split = make_stage(fields, pulldown, pulldown_cycle, self.spec.inp, self.spec.size, deinterlacer, field_rate, combed, comb_threshold,
                                 comb_pixels)          # the stage in front; None: as it was
        for name, value, stage, call in (("denoise_strength", denoise_strength, denoise, "denoise_kwargs"),
                                         ("spatial_strength", spatial_strength, spatial_denoise, "spatial_kwargs")):
            if _auto_strength(value) and stage is not None:          # (without the stage: the options' own refusal, below)
                raise ValueError(f"{name} = 'auto' in VideoUpscaler: the decision needs the whole video; measure the noise first "
                                 f"(savsr_amd.estimate_noise on a probe chunk) and give its {call}(), or use python -m savsr_amd.upscale "
                                 f"--{name.replace('_', '-')} auto")
        # the temporal denoiser, behind that stage (it needs progressive frames) and in front of the crop; None: as it was
        self._noise = make_denoiser(denoise, denoise_radius, denoise_strength, denoise_chroma_strength, self.spec.inp, self.spec.size)
        # the spatial denoiser, behind the crop: stateless, every frame on its own; None: as it was
        self._grain = check_spatial_options(spatial_denoise, spatial_patch, spatial_search, spatial_strength, spatial_chroma_strength)
        # deblocking, on the chunks as pushed: stateless, field by field where the video is interlaced or telecined; None: as it was
        if deblock_grid == "auto":
            raise ValueError("deblock_grid = 'auto' in VideoUpscaler: the decision needs the whole video; find the grid first "
                             "(savsr_amd.detect_grid) and give its kwargs(), or use python -m savsr_amd.upscale --deblock-grid auto")
        self._edges = check_deblock_options(deblock, deblock_block, deblock_strength, deblock_chroma_strength, origin=deblock_origin,
                                            chroma_origin=deblock_chroma_origin, grid=deblock_grid)
        self._fieldwise = fields is not None or pulldown is not None
        self._grid = None if self._edges is None else check_origins(deblock_origin, deblock_chroma_origin, self._edges[0], self._fieldwise,
                                                                    self.spec.inp.layout, "deblock_")
        # deringing, right behind it: stateless, field by field when the deblocker would be; None: as it was
        self._rings = check_dering_options(dering, dering_strength, dering_chroma_strength, dering_damping)
        self._rect = _check_crop_args(crop, 24, bars, auto_ok=False)          # the rect to crop every chunk to; None: no crop, as it was
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
        # surfaces on either side: chunks are unpacked as they arrive and returned frames packed as they leave (stateless: any chunking)
        self._in_tab = None if surface is None else surface_table(surface, self._full.inp, self._full.size)
        self._out_tab = None
        if out_surface is not None:
            surface_side(out_surface, self._full.out, "out_surface")
            if self._full.size:            # (packed input carries its size in the first chunk: the table is resolved there)
                self._set_out_tab(out_surface, *self._full.size)
        self._out_surface = out_surface

    def _set_rect(self, h: int, w: int) -> None:
        """The rect against the full frame size, known now: refused if it does not fit; the whole frame is the uncropped path."""
        rect = active.check_rect(self._rect, h, w, self._full.inp.layout)
        if rect == (0, 0, h, w):
            self._rect = None
            return
        self._rect, self._hw = rect, (h, w)
        self.spec = _cropped_spec(self._full, rect)

    def _set_out_tab(self, out_surface, h: int, w: int) -> None:
        self._out_hw = _out_hw(h, w, self._rect, self.bars, self.scale)
        self._out_tab = surface_table(out_surface, self._full.out, self._out_hw, "out_surface")

    def _emit(self, res: torch.Tensor) -> torch.Tensor:
        """What push() and finish() return: the frames as they are, or packed into out_surface."""
        if self._out_surface is None:
            return res
        return _pack_surface_device(res, self._out_tab, self._full.out, self._out_hw)

    @property
    def pulldown_info(self) -> Optional[dict]:
        """{"matches", "kept"} of the frames pushed so far: per source frame -1 (its second field came from its predecessor) or 0, and the
        indices of the woven frames that went on (None without pulldown=); with combed= also "combed", the woven frames cleaned so far."""
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
        """The SR frames of windows (video indices, all buffered); no window: no frames."""
        if not windows:
            return self._empty()
        with torch.no_grad():
            res = self.net.engine().forward_video(self._buf, [[j - self._base for j in win] for win in windows], self.scale, self.spec,
                                                  ensemble=self.ensemble)
            if self._rect is not None and self.bars == "keep":
                res = _insert_device(res, active.place(self._rect, *self._hw, self.scale, self._full.out.layout), self._full)
            return res

    def _run(self, upto: int, n_total: Optional[int]) -> torch.Tensor:
        """SR frames [done, upto); windows at the video length n_total (None: not known yet, every window needed is interior)."""
        n = n_total if n_total is not None else upto + self.half + 1
        res = self._forward([window_indices(i, n, self.T, self.padding) for i in range(self.done, upto)])
        self.done = upto
        return res

    def _admit(self, frames: torch.Tensor) -> torch.Tensor:
        """One pushed chunk's checks, once per push, in the order they always spoke; returns the chunk on the network's GPU.  The frame
        layout (with a stage in front the stage's own refusals first: float frames, one-row matrices), shape continuity, the first
        chunk's rect, the device.  With a stage the device and the copy to it speak before continuity and the rect, as they did."""
        staged = self._split is not None
        if self._edges is not None:
            _sample_frames(frames, self._full.inp, self._full.size, "deblock")
        if self._rings is not None:
            _sample_frames(frames, self._full.inp, self._full.size, "dering")
        if staged:
            _field_frames(frames, self._full.inp, self._full.size)
        if self._noise is not None or self._grain is not None:
            _denoise_frames(frames, self._full.inp, self._full.size)
        _, h, w = self._full.frames_hw(frames)
        shape = (frames.dtype == torch.uint8, h, w)
        if staged:
            _net_device(self.net)
        if self._shape is not None and shape != self._shape:
            raise ValueError(f"chunk of {'uint8' if shape[0] else 'float'} {h} x {w} frames after {'uint8' if self._shape[0] else 'float'} "
                             f"{self._shape[1]} x {self._shape[2]} ones")
        if staged:
            frames = _to_device(frames, self.net.gamma.device)
        if self._shape is None and self._rect is not None and not self._full.size:
            self._set_rect(h, w)                   # (packed chunks carry the frame size: the rect is checked against the first one's)
        dev = _net_device(self.net)
        self._shape = shape
        return _to_device(frames, dev)

    def push(self, frames: torch.Tensor) -> torch.Tensor:
        if self._finished:
            raise RuntimeError("push() after finish()")
        if self._in_tab is not None:               # a chunk in a surface: checked against it, copied up and unpacked; planar from here on
            surface_layout(frames, self._in_tab)
            frames = _unpack_surface_device(_to_device(frames, _net_device(self.net)), self._in_tab, self._full.inp, self._full.size)
        new = self._admit(frames)
        if self._out_surface is not None and self._out_tab is None:
            self._set_out_tab(self._out_surface, *self._shape[1:])
        if self._edges is not None:                # the frames as decoded, filtered one by one: no frame is held for it
            new = _deblock_device(new, self._full.inp, self._full.size, *self._edges, self._fieldwise, *self._grid)
        if self._rings is not None:                # right behind the deblocker, stateless as well
            new = _dering_device(new, self._full.inp, self._full.size, *self._rings, self._fieldwise)
        if self._split is not None:                # interlaced / telecined chunks: the progressive frames that are final go on as a chunk of their own
            new = self._split.push(new)
            if int(new.shape[0]) == 0:             # (a first push of one frame, or a cycle not complete yet: nothing is final)
                return self._emit(self._empty())
        if self._noise is not None:                # the frames whose `denoise_radius` successors have arrived go on, denoised
            new = self._noise.push(new)
            if int(new.shape[0]) == 0:
                return self._emit(self._empty())
        return self._emit(self._take(new))

    def _take(self, new: torch.Tensor) -> torch.Tensor:
        """Admitted frames on the device (a chunk, or what the stage made of chunks): cropped, buffered, and the windows now complete run."""
        k = int(new.shape[0])
        new = new.contiguous() if self._shape[0] else new.to(torch.float32).contiguous()
        if self._rect is not None:
            new = _crop_device(new, self._rect, self._full.inp, self._shape[1:])
        if self._grain is not None:                # the frames as the network will see them, filtered one by one: no frame is held for it
            new = _denoise_spatial_device(new, self.spec.inp, self.spec.size, *self._grain)
        self._buf = new if self._buf is None else torch.cat([self._buf, new], 0)
        if self._plan is not None:
            return self._push_scenes(k)
        self.seen += k
        upto = self.done
        while upto < self.seen and self._ready(upto):
            upto += 1
        res = self._run(upto, None)
        self._drop_before(self._keep_from())
        return res

    def _drop_before(self, lo: int) -> None:
        if lo > self._base:
            self._buf = self._buf[lo - self._base:]        # (a view: the next push's cat copies it)
            self._base = lo

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
        sad = _pair_sad_device(self._buf[first - 1 - self._base:], self.spec.inp, self.i420).cpu().tolist()
        new = scenes.cuts_from_sad(sad, scenes.sad_samples(self._buf.shape, self.spec.inp.fmt, self.i420), self._threshold, first, self._prev_sad)
        self._prev_sad = sad[-1]
        return new

    def _push_scenes(self, k: int) -> torch.Tensor:
        plan = self._plan
        plan.push(k, self._new_cuts(k))
        self.seen = plan.seen
        res = self._forward(plan.take())
        self.done = plan.done
        lo = plan.keep_from()
        self._drop_before(min(lo, self.seen - 1) if self._auto else lo)          # (auto: the next push's first pair)
        return res

    def finish(self) -> torch.Tensor:
        if self._finished:
            raise RuntimeError("finish() called twice")
        self._finished = True
        last = None if self._split is None else self._split.finish()          # the held source frame's two fields, then the end as ever
        if self._noise is not None:                # they go through the denoiser, which then hands back the frames it held
            parts = [] if last is None or int(last.shape[0]) == 0 else [self._noise.push(last)]
            parts = [p for p in parts + [self._noise.finish()] if p is not None and int(p.shape[0])]
            last = torch.cat(parts, 0) if parts else None
        if last is not None:
            head = self._take(last)
            return self._emit(torch.cat([head, self._finish()], 0))
        return self._emit(self._finish())

    def _finish(self) -> torch.Tensor:
        if self.seen == 0:
            raise ValueError("the video has no frames")
        if self._plan is not None:
            if self._given:
                raise ValueError(f"cut {self._given[0]}: a cut is the first frame of a new scene, 0 < k < {self.seen}")
            self._plan.end()
            res = self._forward(self._plan.take())
            self.done = self._plan.done
            self._buf = None
            return res
        check_length(self.seen, self.T, self.padding)
        res = self._run(self.seen, self.seen)
        self._buf = None
        return res

    def _empty(self) -> torch.Tensor:
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
