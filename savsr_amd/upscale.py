"""Command-line upscaler: LR frames in, SR frames out, as a folder of PNGs or as YUV4MPEG2 (.y4m) video on a file or a pipe.

    python -m savsr_amd.upscale -i <lr_frames/> -o <sr_frames/> --scale 4 --checkpoint <net.pth>
    python -m savsr_amd.upscale -i <lr_frames/> -o <sr_frames/> --scale 3.5 2.5 --padding reflection --opt <test.yml>
    python -m savsr_amd.upscale -i <lr_frames/> -o <sr_frames/> --scale 4 --checkpoint <net.pth> --self-ensemble
    python -m savsr_amd.upscale -i in.y4m -o out.y4m --scale 4 --checkpoint <net.pth>
    ffmpeg -i in.mp4 -f yuv4mpegpipe - | python -m savsr_amd.upscale -i - -o - --scale 4 --checkpoint <net.pth> | ffmpeg -i - out.mp4
    python -m savsr_amd.upscale -i in.y4m -o out.y4m --scale 4 --checkpoint <net.pth> --cuts auto --cuts-out cuts.txt
    python -m savsr_amd.upscale -i sd.y4m -o hd.y4m --scale 4 --checkpoint <net.pth> --colour auto --out-colour auto
    python -m savsr_amd.upscale -i in8.y4m -o out10.y4m --scale 4 --checkpoint <net.pth> --out-depth 10
    ffmpeg -i in.mp4 -f yuv4mpegpipe - | python -m savsr_amd.upscale -i - -o - --scale 4 --checkpoint <net.pth> --siting auto --out-siting same | ffmpeg -i - out.mp4
    python -m savsr_amd.upscale -i in.y4m -o out.y4m --scale 4 --opt <luma_test.yml> --chroma-filter bicubic
    ffmpeg -i pal_dv.avi -f yuv4mpegpipe - | python -m savsr_amd.upscale -i - -o out50p.y4m --scale 4 --checkpoint <net.pth> --fields auto
    python -m savsr_amd.upscale -i letterboxed_sd.y4m -o hd.y4m --scale 4 --checkpoint <net.pth> --crop auto --colour auto --out-colour auto
    python -m savsr_amd.upscale -i dvd_rip.y4m -o out.y4m --scale 4 --checkpoint <net.pth> --scan detect --scan-out scan.json
    ffmpeg -i vhs_capture.avi -f yuv4mpegpipe - | python -m savsr_amd.upscale -i - -o out.y4m --scale 4 --checkpoint <net.pth> --fields auto --denoise ata --denoise-strength 4,9
    ffmpeg -i grainy_sd.avi -f yuv4mpegpipe - | python -m savsr_amd.upscale -i - -o out.y4m --scale 4 --checkpoint <net.pth> --spatial-denoise nlm --spatial-strength 3
    python -m savsr_amd.upscale -i blocky_dvd.y4m -o out.y4m --scale 4 --checkpoint <net.pth> --scan detect --deblock strong --deblock-strength 25,13
    python -m savsr_amd.upscale -i ringing_dvd.y4m -o out.y4m --scale 4 --checkpoint <net.pth> --deblock strong --dering cdef --dering-strength 4,2
    ffmpeg -i in.mov -pix_fmt yuv422p10le -strict -1 -f yuv4mpegpipe - | python -m savsr_amd.upscale -i - -o out444p10.y4m --scale 4 --checkpoint <net.pth> --out-chroma 444

PNG folder: frames are taken in the order read_img_seq reads a folder (sorted scandir, lbasicsr/data/data_util.py:29-60), decoded on
the FrameStore pool (savsr_amd.io), pushed through VideoUpscaler in chunks (uint8 in, uint8 out: the windows, the network and the
quantisation run on the GPU) and encoded on a writer pool of this tool's own (at most 16 threads).

Y4M (a name ending in .y4m, or - for stdin / stdout; savsr_amd/y4m.py): planar YUV 4:2:0 bytes go to the GPU and come back as they are
(pixel_format / out = "i420", "i422" or "i444": colour conversion, chroma resampling and the one rounding happen there, savsr_amd/yuv.py).  On a pipe the
video's length is not known, so a video too short for the window is refused when the input ends.  The SR frames are copied into pinned
buffers and written by one ordered writer thread while the next chunk runs.  The two kinds mix: .y4m in, folder out writes %08d.png;
folder in, .y4m out takes its frame rate from --fps.

--colour / --out-colour: the colour space of the Y4M input / output, one of bt601, bt709 (limited range), bt601-full, bt709-full.  The
defaults (bt601, and the same for the output) are what this tool has always done, so an existing command line writes the bytes it
wrote.  Y4M has no tag for the matrix, and every player and encoder takes an untagged HD stream for BT.709: `auto` follows that
convention (BT.709 if w >= 1280 or h > 576, else BT.601, on the frame size of that side -- players' rule for untagged streams, not a
tuned number) and takes the range from the input's XCOLORRANGE tag (limited without one).  For SD -> HD work give
--colour auto --out-colour auto: the SD source is read as BT.601 and the HD result is written as the BT.709 a player will assume, at
no extra cost and without another 8-bit rounding (the network works in RGB).  The output carries XCOLORRANGE when it is full range or
when either flag was given.

--out-depth: the bit depth of a Y4M output, 8, 10, 12 or same (the default: the input's; 8 for a PNG folder).  A 10- or 12-bit Y4M input
(C420p10 / C420p12, what `ffmpeg -f yuv4mpegpipe` emits for a 10-bit source) is read as it is; its depth comes from the header.  8-bit in,
--out-depth 10 costs nothing extra in the network and keeps the two bits the 8-bit rounding throws away (what HEVC / AV1 encoders take
by default is yuv420p10).  10 and 12 bits go with limited range only: a full-range colour space on a high-depth side is refused.

--out-chroma: the chroma layout of a Y4M output, 420, 422, 444 or same (the default: the input's; 4:2:0 for a PNG folder).  A 4:2:2 or
4:4:4 Y4M input (C422, C444 and their p10 / p12 forms) is read as it is; its layout comes from the header.  The two sides are
independent: 4:2:0 in, --out-chroma 444 writes the network's full-resolution chroma instead of box-filtering it 2 x 2.

--siting / --out-siting: where the chroma samples of a 4:2:0 / 4:2:2 Y4M input / output lie: centre (JPEG, MPEG-1; C420jpeg), left
(MPEG-2, H.264, HEVC 4:2:0 and every standard 4:2:2; C420mpeg2: what `ffmpeg -f yuv4mpegpipe` tags such streams) or topleft (C420paldv;
4:2:0 only).  With a siting, input chroma is interpolated linearly at the positions it names and output chroma is filtered to them
(savsr_amd/yuv.py).  The defaults are none: nearest replication in, block mean out, so an existing command line writes the bytes it
wrote.  --siting auto takes what the input's C tag names (none for a plain C420, a missing tag, C422, C444 and the p10 / p12 tags) and
says on stderr what it resolved to; --out-siting same is whatever the input side resolved to.  An 8-bit 4:2:0 output is tagged
C420mpeg2 / C420paldv for left / topleft and C420jpeg otherwise.

--chroma-filter bicubic: a luma-only checkpoint (num_in_ch = 1, from --opt) on a Y4M input: the Y plane goes through the network and
Cb / Cr are resampled from each frame's own chroma planes at the network's scale by a siting-aware bicubic (savsr_amd/yuv.py "Luma-only
checkpoints"); --out-depth, --out-chroma, --siting and --out-siting apply, the colour space is kept.  The default, none, is what this tool
has always done.  A grey-scale input (Cmono, Cmono10, Cmono12) needs such a checkpoint and no filter, and is written as grey-scale.

--dither ordered: 8-bit output of smooth gradients (sky, vignettes, fades), which a x4 result stretches into bands four times as wide.
Every integer output -- the PNG folder, and Y, Cb and Cr of a Y4M output at any depth -- is written as floor(t + theta) instead of
rint(t), theta a threshold from a 16 x 16 Bayer matrix at the sample's position (savsr_amd/dither.py), so that the mean over every
16 x 16 block keeps the fp32 result to 1/256 of a code.  The pattern is static in time and the same for any --chunk.  The default, none,
writes the bytes this tool has always written.  With --chroma-filter the resampled Cb / Cr keep rint.

--cuts: edited footage.  Windows stop at scene cuts (every scene is upscaled as a video of its own, savsr_amd/scenes.py): auto finds
them on the GPU as the frames arrive (--scene-threshold, per cent of the largest possible frame change; ffmpeg scdet's rule and default,
not validated on real footage), K,K,... or @FILE (one frame index per line) gives them.  --cuts-out FILE writes the cuts used, one per line.

--crop: letterboxed, pillarboxed and window-boxed footage.  The frames are cropped to the active picture before anything else sees
them (savsr_amd/active.py), so the bars cost no network time and stay out of the network's global pools.  auto makes a first pass over a
.y4m file or a PNG folder in --chunk-sized pieces (line sums on the GPU, a running maximum there), applies ffmpeg cropdetect's rule with
--crop-limit (the largest mean of a black line on the 8-bit scale; cropdetect's default, 24, not validated on real footage) and reports
the rect on stderr; on stdin there is no second pass, so give Y0,X0,H,W there.  --bars keep (the default) writes full-size frames with
the picture in nominal black; --bars drop writes the picture alone, and a Y4M output then carries the picture's size.

--fields: interlaced footage (PAL / NTSC broadcast, DV, DVD video that is not film).  The frames are deinterlaced on the GPU into
progressive frames at the field rate before anything else sees them (savsr_amd/deinterlace.py: ffmpeg yadif's rule; every source frame
gives two), so the network's windows, --cuts and --crop work on pictures and not on woven fields; K in --cuts K,... and Y0,X0,H,W index and
measure the deinterlaced video.  tff / bff name the field order, auto takes it from the Y4M input's I tag (It -> tff, Ib -> bff, Ip ->
progressive; Im, mixed, is refused).  The output is then tagged Ip at twice the frame rate, and a PNG folder holds twice the files
(%08d.png).  The default, progressive, is what this tool has always done: the frames go through as they are and the I tag is passed on;
for an input tagged It / Ib / Im one line on stderr says so.  Telecined film is not interlaced video: see --pulldown.
--deinterlacer bwdif interpolates by ffmpeg bwdif's rule instead (still areas come back as they are); --field-rate same keeps the first
field in time of every frame only: the output is tagged Ip at the input's frame rate, a PNG folder holds as many files as were read, and
the network runs once per input frame.  Both go with --fields or --scan detect.

--pulldown: telecined film (3:2 pulldown: most NTSC film DVDs and broadcast film; four film frames lie in five video frames as the fields
AA BB BC CD DD).  The film frames are recovered on the GPU before anything else sees them (savsr_amd/pulldown.py: every frame keeps its
first field and takes the second from itself or from the frame before it, whichever combs less; of every --pulldown-cycle (default 5)
woven frames the one closest to its predecessor is dropped), so the network runs 4 frames for every 5 read; K in --cuts K,... indexes the
film frames.  tff / bff name the field order, auto takes it from the Y4M input's I tag as --fields auto does (Im is refused).  The
output is tagged Ip at (cycle - 1) / cycle of the frame rate (30000:1001 -> 24000:1001), and a PNG folder holds the kept frames
(%08d.png).  Not together with --fields tff / bff / auto: they are two answers to one question.  There is no cadence tracking: a cadence
broken by an edit costs one real frame in that cycle, and a frame that matches neither neighbour stays combed unless --combed is given.

--combed yadif / bwdif: hybrid material (film with video-rate titles or effects, series cut on tape, a stream that starts or is cut
inside a cadence).  After the field match every woven frame is measured for residual combing (savsr_amd.comb_windows: a sample is combed
when its comb measure exceeds twice --comb-threshold, a frame when some 16 x 16 window, one every 8 rows and pixels, holds --comb-pixels
of them); the combed frames alone are deinterlaced at same rate by that rule and the decimation reads the cleaned frames (ffmpeg's
fieldmatch -> yadif=deint=interlaced -> decimate chain).  One line on stderr says how many frames were cleaned.  Goes with --pulldown or
--scan detect (a telecine verdict; ignored for the others).  The decimation still drops one of every five frames of a true-video insert
(judder, not combing), a cleaned frame has half its rows interpolated, and small or low-contrast combing stays below the rule; the
defaults (9, 40) are fieldmatch's and are not validated on footage.

--scan detect: footage whose scan is not known, or whose tag is not trusted (encoders tag hard-telecined film and much progressive
material It; a PNG folder has no tag at all).  A first pass over a .y4m file or a PNG folder in --chunk-sized pieces computes the field
statistics on the GPU (savsr_amd/scan.py: comb measures of every frame's fields against its own and its neighbours' fields, and the SAD
of each field against the previous frame's), the host decides -- the 3:2 cadence of repeated fields first, then whether a frame's two
fields fit each other better than its neighbours' (progressive), then which field order fits (interlaced) -- and one line on stderr
names the verdict and the equivalent flag, e.g. "--scan detect: telecine, bottom field first: --pulldown bff".  The run then goes on as
--fields X / --pulldown X would (or as without them for progressive video and for video that shows no evidence: static, flat); when the
input's I tag says something else, one more line says so.  --scan-out FILE writes the verdict as JSON (scan, order, totals, hits, the
per-frame repeated field).  Not on stdin (there is no second pass: give --fields or --pulldown there) and not together with --fields or
--pulldown.  The rule and its thresholds are this project's own and are not validated on real footage; one verdict per video: mixed
content, 2:2 PAL film, cadences other than 3:2 and fades are not handled.

--denoise ata: noisy footage (tape and tuner noise, sensor noise, the temporal flicker MPEG-2 quantisation leaves), which a network
trained on clean downsamples enlarges as detail.  Every sample is averaged on the GPU with the same sample of up to --denoise-radius N
(default 4: nine frames; 1 .. 16) frames on either side, in two independent walks that each take the next frame's sample while it
differs by at most A and the walk's differences sum to at most B (--denoise-strength A,B in 8-bit code units at every depth, default
4,9; ffmpeg atadenoise's serial rule, savsr_amd/denoise.py); --denoise-chroma-strength A,B sets the chroma planes of a Y4M input apart.
The stage runs behind --fields / --pulldown / --scan detect (it needs progressive frames) and in front of --crop and --cuts, which see
the denoised frames; N frames are held back and flushed at the end, and one line on stderr names the stage and its parameters.  Works
for PNG folders and for .y4m files and pipes.  Temporal only: moving texture is not denoised, the taps read across scene cuts (only the
thresholds stop them), one strength per video; the defaults are parameters and nothing is validated on footage.

--spatial-denoise nlm: grain, tuner and sensor noise on what moves, which --denoise (temporal only) leaves untouched.  Non-local means
on the GPU, every frame on its own: a sample becomes the weighted mean of the samples within --spatial-search N (default 7: a 15 x 15
window; 1 .. 7) of it, each weighted by how alike the (2 P + 1)^2 patches around the two are (--spatial-patch P, default 3; 1 .. 3);
--spatial-strength H (default 3.0, 0 < H <= 32, 8-bit code units at every depth) is the root mean squared patch difference at which the
weight is 1 / e (savsr_amd/nlmeans.py); --spatial-chroma-strength H sets the chroma planes of a Y4M input apart.  The stage runs behind
--denoise and behind --crop (the bars never enter a patch), in front of --cuts; no frame is held back, and one line on stderr names the
stage and its parameters.  Works for PNG folders and for .y4m files and pipes.  One strength per video, no joint-channel weights, the
search stops at 15 x 15; the defaults are parameters, nothing is validated on footage and nothing is pinned to ffmpeg's nlmeans.

--denoise-strength auto / --spatial-strength auto: the strength from the noise level of the input (savsr_amd/noise.py: the 8 x 8 cell
sums of an absolute 3 x 3 second difference on the GPU, the mean of the quietest quarter of the cells on the host).  Each is a first
pass of its own over a .y4m file or a PNG folder, in --chunk pieces, through the stages in front of its measuring point as the second
pass will run them (--deblock, --dering, --fields / --pulldown; for the spatial one also --denoise at the strength just found, and the
crop): the passes run in the order scan, grid, temporal noise, crop, spatial noise.  One line on stderr per pass gives the verdict and
the equivalent flags; where no noise is found (sigma below half a code) that is --denoise none / --spatial-denoise none and the stage is
left out.  --noise-out FILE writes both verdicts as JSON (sigma per class, cells, flat cells, the summed tables, the chosen flags).  An
explicit --denoise-chroma-strength / --spatial-chroma-strength wins over the found one.  Not on stdin (there is no second pass).  The
measure, its constants and the gains are this project's own and are not validated on footage.

--deblock weak|strong: the 8 x 8 block edges of MPEG-2 and low-bitrate H.264 sources, which neither denoiser removes.  On the GPU, every
frame on its own: across the vertical edges of a grid of --deblock-block N (default 8; 4, 8 or 16) samples whose first edges lie at
--deblock-origin Y,X (default 0,0), then across the horizontal ones, the 2 (weak) or 3 (strong) samples on either side of an edge move towards each other where the
step across it is below A and the steps beside it are below B (--deblock-strength A,B in 8-bit code units at every depth, default
25,13, ints in 0 .. 255; savsr_amd/deblock.py); --deblock-chroma-strength A,B sets the chroma planes of a Y4M input apart.  The grid
belongs to the coded frame, so the stage runs on the frames as read, in front of --fields / --pulldown, --denoise, --crop (auto reads
the filtered frames), --spatial-denoise and --cuts, and field by field where the video is treated as interlaced: with --fields or
--pulldown, or an interlaced or telecine verdict of --scan detect, whose first pass reads the unfiltered frames.  No frame is held back,
and one line on stderr names the stage, its parameters and whether it ran field-wise.  Works for PNG folders and for .y4m files and
pipes.  A video whose bars or overscan were cropped by c samples before it arrived has its edges at (-c) mod N: --deblock-origin Y,X says
so (Y even where the stage runs field-wise), --deblock-chroma-origin Y,X for the chroma planes of a Y4M input in chroma samples (4:2:0 /
4:2:2 input with an origin other than 0,0 must name it).  --deblock-grid auto finds block size and origins from the frames instead
(savsr_amd/grid.py): a first pass over a .y4m file or a PNG folder in --chunk pieces, the statistics summed on the GPU -- behind
--scan detect's pass, whose verdict says whether to count field-wise, and in front of --crop auto's -- then an exact rule on the host;
one line on stderr gives the verdict and the equivalent flags, --grid-out FILE writes it as JSON (block, origins, the summed table, the
peaks); no grid found: the stage is left out; chroma planes that show no grid of the luma's block are left alone.  It is refused on
stdin and together with --deblock-block / --deblock-origin.  The detector's rule and defaults are this project's own and are not
validated on footage; grids of scaled video, other block sizes and block 4 on noise-free material are not found.  One grid and one strength per video, no adaptation to the stream's quantiser; the
defaults are parameters, nothing is validated on footage and nothing is pinned to ffmpeg's deblock.

--dering cdef: the ringing and mosquito noise a coarsely quantised 8 x 8 DCT puts around sharp edges, which --deblock and both denoisers
leave.  On the GPU, every frame on its own: every 8 x 8 block of a plane (the grid starts at the plane's origin) gets one of eight
directions from its line sums, and every sample moves by a constrained sum of four taps along its block's direction and eight across it,
clamped to the minimum and maximum of the sample and its taps (--dering-strength P,S in 8-bit code units at every depth, default 4,2,
0 <= P <= 15 along and 0 <= S <= 4 across; --dering-damping N, default 5, 3 .. 6: a tap whose difference is large against its strength
counts less; savsr_amd/dering.py; the idea is that of AV1's CDEF, the definition this project's); --dering-chroma-strength P,S sets the
chroma planes of a Y4M input apart.  Ringing belongs to the coded frame, so the stage runs on the frames as read right behind --deblock,
in front of --fields / --pulldown, --denoise, --crop (auto reads the filtered frames), --spatial-denoise and --cuts, and field by field
where the video is treated as interlaced, as --deblock does.  No frame is held back, and one line on stderr names the stage, its
parameters and whether it ran field-wise.  Works for PNG folders and for .y4m files and pipes.  One strength per video, no per-block
signalling such as a bitstream carries, the 8 x 8 grid does not follow --deblock-origin, chroma gets a direction of its own, fine noise
is smoothed too; the defaults are parameters, nothing is validated on footage and nothing is pinned to libaom's or ffmpeg's output.

It ends with one line: frames, seconds, frames/s (on stderr when the video goes to stdout); with --cuts, the scene count as well; with
--colour / --out-colour, the two colour spaces.
"""
from __future__ import annotations

import argparse
import os
import queue
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional

from . import deblock as dbk
from . import dering as drg
from .denoise import DEFAULT_RADIUS, DEFAULT_STRENGTH, DENOISERS, MAX_RADIUS, check_radius, check_strength
from .dither import DITHERS
from . import nlmeans as nlm
from .deinterlace import DEINTERLACERS, FIELD_FLAGS, FIELD_ORDERS, FIELD_RATES, resolve_fields
from .pulldown import (DEFAULT_COMB_PIXELS, DEFAULT_COMB_THRESHOLD, DEFAULT_CYCLE, PULLDOWN_FLAGS, check_comb_pixels, check_comb_threshold, check_cycle,
                       resolve_pulldown)
from .scan import SCAN_FLAGS
from .yuv import COLOURS, SITINGS

MAX_WRITERS = 16
PINNED_BUFFERS = 3          # SR chunks in flight between the GPU and the Y4M writer thread


def is_y4m(path: str) -> bool:
    return path == "-" or path.lower().endswith(".y4m")


def auto_colour(h: int, w: int, full: bool) -> str:
    """The colour space players assume of an untagged h x w stream: BT.709 if w >= 1280 or h > 576, else BT.601; `full`: its range."""
    return ("bt709" if w >= 1280 or h > 576 else "bt601") + ("-full" if full else "")


def resolve_colours(colour: str, out_colour: str, lr, hr, in_range: Optional[str]):
    """--colour / --out-colour -> (colour of the Y4M input or None, colour of the Y4M output or None).  lr / hr: (h, w) of a Y4M input /
    output, None for a PNG folder on that side; in_range: the input's XCOLORRANGE ("full", "limited" or None = limited).  An output
    `auto` takes the range the input was read with (limited for PNGs); `same` is the input's colour space (bt601 for PNGs)."""
    from .yuv import is_full_range
    cin = None
    if lr is not None:
        cin = auto_colour(lr[0], lr[1], in_range == "full") if colour == "auto" else colour
    cout = None
    if hr is not None:
        if out_colour == "same":
            cout = cin or "bt601"
        elif out_colour == "auto":
            cout = auto_colour(hr[0], hr[1], cin is not None and is_full_range(cin))
        else:
            cout = out_colour
    return cin, cout


def resolve_sitings(siting: str, out_siting: str, tag_siting: Optional[str], chroma: Optional[str], out_chroma: Optional[str]):
    """--siting / --out-siting -> (siting of the Y4M input, siting of the Y4M output), each None or one of yuv.SITINGS.  tag_siting: what
    the input's C tag names (Y4MReader.siting); chroma / out_chroma: the layout of a Y4M input / output, None for a PNG folder on that
    side.  `auto` is the tag's; `same` is what the input side resolved to.  4:4:4 has nothing to resample: a siting there resolves to
    None.  topleft on a 4:2:2 side is refused (ValueError)."""
    from .yuv import check_siting
    sin = None
    if chroma is not None:
        sin = tag_siting if siting == "auto" else (None if siting == "none" else siting)
        if chroma == "444":
            sin = None
        check_siting(sin, chroma, "--siting")
    sout = None
    if out_chroma is not None:
        sout = sin if out_siting == "same" else (None if out_siting == "none" else out_siting)
        if out_chroma == "444":
            sout = None
        check_siting(sout, out_chroma, "--out-siting")
    return sin, sout


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m savsr_amd.upscale", description="Upscale LR video frames (a folder of PNGs, or YUV4MPEG2) with SAVSR.")
    p.add_argument("-i", "--input", required=True, help="folder of LR frames (PNG), taken in sorted order; or a .y4m file; or - (Y4M on stdin)")
    p.add_argument("-o", "--output", required=True,
                   help="output folder (created; SR frames keep the input file names, %%08d.png for a Y4M input); or a .y4m file; or - (Y4M on stdout)")
    p.add_argument("--fps", default=None, metavar="N[:D]", help="frame rate of a Y4M output made from a PNG folder (default 25:1)")
    p.add_argument("--scale", type=float, nargs="+", required=True, metavar="S", help="s, or sh sw")
    p.add_argument("--padding", default="reflection", choices=["replicate", "reflection", "reflection_circle", "circle"],
                   help="window padding at the ends of the video (generate_frame_indices); default reflection")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--opt", help="test YAML: network_g and path.pretrain_network_g / param_key_g / strict_load_g")
    src.add_argument("--checkpoint", help="checkpoint (.pth, 'params' key) for SAVSR with default constructor arguments")
    p.add_argument("--chunk", type=int, default=16, help="frames per push (default 16)")
    p.add_argument("--writers", type=int, default=0, help=f"PNG encoder threads (default: the usable CPUs, at most {MAX_WRITERS})")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--precision", default="fp32", choices=["fp32", "fp16"],
                   help="conv operand precision (default fp32; fp16: faster, ~1e-3 drift, see DESIGN.md section 3)")
    p.add_argument("--self-ensemble", action="store_true",
                   help="average the 8 flip / transpose variants of every window (8x the work; DESIGN.md section 11)")
    p.add_argument("--colour", default=None, choices=list(COLOURS) + ["auto"],
                   help="colour space of a Y4M input (default bt601, limited range).  auto: the range from the input's XCOLORRANGE tag (limited "
                        "without one) and the matrix players assume of an untagged stream of that size: bt709 if w >= 1280 or h > 576, else bt601")
    p.add_argument("--out-colour", default=None, choices=list(COLOURS) + ["auto", "same"],
                   help="colour space of a Y4M output (default same: the input's; bt601 for a PNG folder).  auto: the input's range and the matrix "
                        "players assume at the output size.  For SD -> HD give --colour auto --out-colour auto: an untagged HD stream is shown as "
                        "BT.709, so a BT.601 one has shifted colours")
    p.add_argument("--out-depth", default=None, choices=["8", "10", "12", "same"],
                   help="bit depth of a Y4M output (default same: the input's; 8 for a PNG folder).  10 / 12 write C420p10 / C420p12, limited range "
                        "only; 8-bit in, 10 out keeps the precision the 8-bit rounding loses")
    p.add_argument("--out-chroma", default=None, choices=["420", "422", "444", "same"],
                   help="chroma layout of a Y4M output (default same: the input's; 420 for a PNG folder).  422 / 444 write C422 / C444 "
                        "(C422p10 ... with --out-depth 10 / 12); 444 keeps the network's full-resolution chroma")
    p.add_argument("--siting", default=None, choices=["none", "auto"] + list(SITINGS),
                   help="chroma siting of a 4:2:0 / 4:2:2 Y4M input (default none: not modelled, nearest replication).  auto: what the input's "
                        "C tag names (C420jpeg centre, C420mpeg2 left, C420paldv topleft, none otherwise), reported on stderr; with a siting, "
                        "chroma is interpolated linearly at its positions")
    p.add_argument("--out-siting", default=None, choices=["none", "same"] + list(SITINGS),
                   help="chroma siting of a 4:2:0 / 4:2:2 Y4M output (default none: block mean).  same: what the input side resolved to; "
                        "left / topleft filter cosited axes with [1 2 1] / 4 and tag an 8-bit 4:2:0 output C420mpeg2 / C420paldv")
    p.add_argument("--chroma-filter", default="none", choices=["none", "bicubic"],
                   help="luma-only checkpoints (num_in_ch = 1) on Y4M video: bicubic resamples Cb / Cr from the input's chroma planes at the "
                        "network's scale while Y goes through the network (default none)")
    p.add_argument("--dither", default="none", choices=["none"] + list(DITHERS),
                   help="how the fp32 result becomes integer codes (PNG folders and Y4M alike).  none (default): round to nearest; ordered: "
                        "floor(t + theta) with a 16 x 16 Bayer threshold at the sample's position, which keeps smooth gradients from banding "
                        "at 8 bits (static in time)")
    p.add_argument("--cuts", default=None, metavar="auto|K,K,...|@FILE",
                   help="scene cuts (first frame of every new scene): auto = found on the GPU, a comma-separated list, or @FILE with one index "
                        "per line; windows stop at cuts")
    p.add_argument("--scene-threshold", type=float, default=10.0, metavar="X",
                   help="--cuts auto: a cut is a frame change of at least X per cent of the largest possible one (default 10, ffmpeg scdet's)")
    p.add_argument("--cuts-out", default=None, metavar="FILE", help="write the cut list actually used, one frame index per line")
    p.add_argument("--crop", default=None, metavar="auto|Y0,X0,H,W",
                   help="upscale the active picture alone: auto = found on the GPU in a first pass over the input (a file or a folder), or the "
                        "rect's top-left corner and size in LR pixels")
    p.add_argument("--crop-limit", type=float, default=None, metavar="X",
                   help="--crop auto: a row or column whose mean stays at or below X (8-bit scale) in every frame is bar (default 24, ffmpeg "
                        "cropdetect's; not validated on real footage)")
    p.add_argument("--fields", default=None, choices=list(FIELD_FLAGS),
                   help="interlaced input: deinterlace on the GPU first, every frame giving two progressive ones at the field rate.  tff / bff: "
                        "the field order; auto: from the Y4M input's I tag (It, Ib; Im is refused); progressive (default): frames go through as "
                        "they are, the I tag is passed on")
    p.add_argument("--deinterlacer", default=None, choices=list(DEINTERLACERS),
                   help="--fields / --scan detect: the rule that interpolates the missing rows.  yadif (default); bwdif: ffmpeg bwdif's rule "
                        "(yadif's temporal clamp around the w3fdif filters), which returns still areas as they are")
    p.add_argument("--field-rate", default=None, choices=list(FIELD_RATES),
                   help="--fields / --scan detect: double (default) = two progressive frames per input frame at the field rate; same = one, "
                        "the first field in time, at the input's frame rate (half the network's work)")
    p.add_argument("--pulldown", default=None, choices=list(PULLDOWN_FLAGS),
                   help="telecined film (3:2 pulldown): recover the film frames on the GPU first, 4 for every 5 read.  tff / bff: the field "
                        "order; auto: from the Y4M input's I tag (It, Ib; Im is refused); none (default): frames go through as they are")
    p.add_argument("--pulldown-cycle", type=int, default=None, metavar="N",
                   help="--pulldown: one frame in every N is the repeated one and is dropped (default 5; 2 .. 25)")
    p.add_argument("--combed", default=None, choices=["none"] + list(DEINTERLACERS),
                   help="--pulldown / --scan detect: hybrid film and video.  yadif / bwdif: woven frames that are still combed (video inserts, "
                        "a stream cut inside a cadence) are deinterlaced at same rate by that rule before the decimation; none (default): "
                        "they stay as they are")
    p.add_argument("--comb-threshold", type=int, default=None, metavar="X",
                   help="--combed: a sample is combed when its comb measure exceeds 2 X (default 9, ffmpeg fieldmatch's cthresh; 0 .. 255; "
                        "not validated on footage)")
    p.add_argument("--comb-pixels", type=int, default=None, metavar="N",
                   help="--combed: a frame is combed when a 16 x 16 window holds N combed pixels (default 40 of 128, fieldmatch's combpel "
                        "80 / 256; 1 .. 128; not validated on footage)")
    p.add_argument("--denoise", default=None, choices=["none"] + list(DENOISERS),
                   help="temporal noise reduction on the GPU in front of the network.  ata: every sample is averaged with the same sample of "
                        "the frames around it while they stay close to it (ffmpeg atadenoise's serial rule); none (default): the frames go "
                        "through as they are")
    p.add_argument("--denoise-radius", type=int, default=None, metavar="N",
                   help=f"--denoise: the frames averaged on either side (default {DEFAULT_RADIUS}: nine frames; 1 .. {MAX_RADIUS})")
    p.add_argument("--denoise-strength", default=None, metavar="A,B",
                   help=f"--denoise: a tap is taken while it differs by at most A and the differences of its side sum to at most B, in 8-bit "
                        f"code units at every depth (default {DEFAULT_STRENGTH[0]},{DEFAULT_STRENGTH[1]}; 0 <= A <= B <= 255; not validated on footage); "
                        f"auto: from the noise level measured in a first pass over the input (savsr_amd/noise.py), no noise found: the stage "
                        f"is left out")
    p.add_argument("--denoise-chroma-strength", default=None, metavar="A,B",
                   help="--denoise: the same for the chroma planes of a Y4M input (default: --denoise-strength)")
    p.add_argument("--spatial-denoise", default=None, choices=["none"] + list(nlm.SPATIAL_DENOISERS),
                   help="spatial noise reduction on the GPU in front of the network, behind --denoise and --crop.  nlm: non-local means, every "
                        "frame on its own; none (default): the frames go through as they are")
    p.add_argument("--spatial-patch", type=int, default=None, metavar="N",
                   help=f"--spatial-denoise: the patch radius (default {nlm.DEFAULT_PATCH}: 7 x 7 patches; 1 .. {nlm.MAX_PATCH})")
    p.add_argument("--spatial-search", type=int, default=None, metavar="N",
                   help=f"--spatial-denoise: the search radius (default {nlm.DEFAULT_SEARCH}: a 15 x 15 window; 1 .. {nlm.MAX_SEARCH})")
    p.add_argument("--spatial-strength", type=float_or_auto, default=None, metavar="H",
                   help=f"--spatial-denoise: the root mean squared patch difference at which the weight is 1 / e, in 8-bit code units at every "
                        f"depth (default {nlm.DEFAULT_STRENGTH}; 0 < H <= {nlm.MAX_STRENGTH}; not validated on footage); auto: from the noise level "
                        f"measured in a first pass over the input, behind --denoise and --crop (savsr_amd/noise.py), no noise found: the stage "
                        f"is left out")
    p.add_argument("--spatial-chroma-strength", type=float, default=None, metavar="H",
                   help="--spatial-denoise: the same for the chroma planes of a Y4M input (default: --spatial-strength)")
    p.add_argument("--deblock", default=None, choices=["none"] + list(dbk.DEBLOCKERS),
                   help="deblocking on the GPU in front of the network, on the frames as read.  weak: 2 samples on either side of a block edge; "
                        "strong: 3; none (default): the frames go through as they are")
    p.add_argument("--deblock-block", type=int, default=None, metavar="N",
                   help=f"--deblock: the block's size in samples (default {dbk.DEFAULT_BLOCK}; 4, 8 or 16; the grid starts at the frame's origin)")
    p.add_argument("--deblock-strength", default=None, metavar="A,B",
                   help=f"--deblock: an edge is filtered where its step is below A and the steps beside it are below B, in 8-bit code units at "
                        f"every depth (default {dbk.DEFAULT_STRENGTH[0]},{dbk.DEFAULT_STRENGTH[1]}; ints in 0 .. 255; not validated on footage)")
    p.add_argument("--deblock-chroma-strength", default=None, metavar="A,B",
                   help="--deblock: the same for the chroma planes of a Y4M input (default: --deblock-strength)")
    p.add_argument("--dering", default=None, choices=["none"] + list(drg.DERINGERS),
                   help="deringing on the GPU in front of the network, on the frames as read, right behind --deblock.  cdef: a direction per "
                        "8 x 8 block, a constrained filter along and across it; none (default): the frames go through as they are")
    p.add_argument("--dering-strength", default=None, metavar="P,S",
                   help=f"--dering: the strength along a block's direction (0 .. {drg.MAX_PRIMARY}) and across it (0 .. {drg.MAX_SECONDARY}), in "
                        f"8-bit code units at every depth (default {drg.DEFAULT_STRENGTH[0]},{drg.DEFAULT_STRENGTH[1]}; not validated on footage)")
    p.add_argument("--dering-chroma-strength", default=None, metavar="P,S",
                   help="--dering: the same for the chroma planes of a Y4M input (default: --dering-strength)")
    p.add_argument("--dering-damping", type=int, default=None, metavar="N",
                   help=f"--dering: a tap whose difference is large against its strength counts less, then not at all; larger N lets larger "
                        f"differences count (default {drg.DEFAULT_DAMPING}; {drg.MIN_DAMPING} .. {drg.MAX_DAMPING})")
    p.add_argument("--scan", default=None, choices=list(SCAN_FLAGS),
                   help="detect: find out from the content, in a first pass over the input (a file or a folder), whether it is progressive, "
                        "interlaced or telecined film and with which field order, then run as --fields X / --pulldown X would; the verdict "
                        "goes to stderr (thresholds not validated on real footage)")
    p.add_argument("--deblock-origin", default=None, metavar="Y,X",
                   help="--deblock: the grid's first edges, 0 <= Y, X < the block (default 0,0; a video cropped by c samples before it arrived "
                        "has them at (-c) mod block; Y even where the stage runs field-wise)")
    p.add_argument("--deblock-chroma-origin", default=None, metavar="Y,X",
                   help="--deblock: the same for the chroma planes of a Y4M input, in chroma samples (4:2:0 / 4:2:2 input with an origin other "
                        "than 0,0 must name it; default: --deblock-origin)")
    p.add_argument("--deblock-grid", default=None, choices=["auto"],
                   help="--deblock: find the block size and the origins from the frames in a first pass over the input (savsr_amd/grid.py; the "
                        "rule's defaults are this project's own and are not validated on footage); no grid found: the stage is left out")
    p.add_argument("--grid-out", default=None, metavar="FILE", help="--deblock-grid auto: write the verdict as JSON")
    p.add_argument("--noise-out", default=None, metavar="FILE",
                   help="--denoise-strength auto / --spatial-strength auto: write the verdicts as JSON (sigma per class, cells, flat cells, the "
                        "summed tables, the chosen flags)")
    p.add_argument("--scan-out", default=None, metavar="FILE", help="--scan detect: write the verdict as JSON")
    p.add_argument("--bars", default=None, choices=["keep", "drop"],
                   help="--crop: keep = full-size output, the picture in nominal black (default); drop = the picture alone")
    return p


def float_or_auto(text: str):
    """--spatial-strength: "auto" or a number."""
    return text if text == "auto" else float(text)


float_or_auto.__name__ = "float"          # (argparse names the type in its refusal: "invalid float value")


def parse_crop(text: str):
    """--crop: "auto" or "Y0,X0,H,W" -> "auto" or a rect of ints (the frame size is checked once it is known)."""
    from .active import check_rect
    if text == "auto":
        return text
    try:
        rect = tuple(int(t.strip()) for t in text.split(","))
    except ValueError:
        raise ValueError(f"auto or Y0,X0,H,W with integers, got {text!r}") from None
    if len(rect) != 4:
        raise ValueError(f"auto or Y0,X0,H,W, got {text!r}")
    return check_rect(rect, None, None, None)


def parse_strength(text: str, what: str):
    """--denoise-strength / --denoise-chroma-strength: "A,B" -> the checked (a, b)."""
    try:
        pair = tuple(int(t.strip()) for t in text.split(","))
    except ValueError:
        raise ValueError(f"{what}: A,B with integers, got {text!r}") from None
    if len(pair) != 2:
        raise ValueError(f"{what}: A,B, got {text!r}")
    return check_strength(pair, what)


def parse_deblock_origin(text: str, block: int, what: str):
    """--deblock-origin / --deblock-chroma-origin: "Y,X" -> the checked (oy, ox)."""
    parts = text.split(",")
    try:
        origin = tuple(int(v) for v in parts)
    except ValueError:
        origin = None
    if origin is None or len(origin) != 2:
        raise ValueError(f"{what} = {text!r}: Y,X, two ints in 0 .. {block - 1}")
    return dbk.check_origin(origin, block, False, what)


def parse_deblock_strength(text: str, what: str):
    """--deblock-strength / --deblock-chroma-strength: "A,B" -> the checked (a, b)."""
    try:
        pair = tuple(int(t.strip()) for t in text.split(","))
    except ValueError:
        raise ValueError(f"{what}: A,B with integers, got {text!r}") from None
    if len(pair) != 2:
        raise ValueError(f"{what}: A,B, got {text!r}")
    return dbk.check_strength(pair, what)


def parse_dering_strength(text: str, what: str):
    """--dering-strength / --dering-chroma-strength: "P,S" -> the checked (p, s)."""
    try:
        pair = tuple(int(t.strip()) for t in text.split(","))
    except ValueError:
        raise ValueError(f"{what}: P,S with integers, got {text!r}") from None
    if len(pair) != 2:
        raise ValueError(f"{what}: P,S, got {text!r}")
    return drg.check_strength(pair, what)


def parse_cuts(text: str):
    """--cuts: "auto", "K,K,..." or "@FILE" (one index per line, blank lines skipped) -> "auto" or a checked list of ints."""
    from .scenes import check_cuts
    if text == "auto":
        return text
    if text.startswith("@"):
        try:
            with open(text[1:]) as f:
                items = [ln.strip() for ln in f if ln.strip()]
        except OSError as e:
            raise ValueError(f"cannot read {text[1:]!r}: {e}") from None
    else:
        items = [t.strip() for t in text.split(",") if t.strip()]
        if not items:
            raise ValueError("an empty list: give auto, K,K,... or @FILE")
    try:
        cuts = [int(t) for t in items]
    except ValueError:
        raise ValueError(f"frame indices are integers, got {items!r}") from None
    return check_cuts(cuts, None)


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    p = build_parser()
    a = p.parse_args(argv)
    if len(a.scale) not in (1, 2):
        p.error("--scale takes one value (s) or two (sh sw)")
    if any(s <= 0 for s in a.scale):
        p.error("--scale must be positive")
    a.scale = (a.scale[0], a.scale[0]) if len(a.scale) == 1 else tuple(a.scale)
    if a.chunk < 1:
        p.error("--chunk must be >= 1")
    if a.writers < 0 or a.writers > MAX_WRITERS:
        p.error(f"--writers must be in 0 .. {MAX_WRITERS}")
    if a.cuts is not None:
        from .scenes import check_threshold
        try:
            a.cuts = parse_cuts(a.cuts)
            check_threshold(a.scene_threshold)
        except ValueError as e:
            p.error(f"--cuts / --scene-threshold: {e}")
    elif a.cuts_out is not None:
        p.error("--cuts-out goes with --cuts")
    if a.crop is not None:
        from .active import DEFAULT_LIMIT, check_limit
        try:
            a.crop = parse_crop(a.crop)
            check_limit(DEFAULT_LIMIT if a.crop_limit is None else a.crop_limit)
        except ValueError as e:
            p.error(f"--crop / --crop-limit: {e}")
        if a.crop_limit is not None and a.crop != "auto":
            p.error("--crop-limit goes with --crop auto (an explicit rect needs no detector)")
        if a.crop == "auto" and a.input == "-":
            p.error("--crop auto needs a first pass over the input, which stdin does not allow: give the rect, --crop Y0,X0,H,W "
                    "(ffmpeg cropdetect or savsr_amd.detect_active_area find it)")
    elif a.crop_limit is not None or a.bars is not None:
        p.error("--crop-limit and --bars go with --crop")
    a.crop_limit = 24 if a.crop_limit is None else a.crop_limit
    if a.scan is not None:
        if a.input == "-":
            p.error("--scan detect needs a first pass over the input, which stdin does not allow: give --fields tff / bff / progressive or "
                    "--pulldown tff / bff (savsr_amd.detect_scan on a probe chunk finds them)")
        if a.fields is not None or a.pulldown is not None:
            given = f"--fields {a.fields}" if a.fields is not None else f"--pulldown {a.pulldown}"
            p.error(f"--scan detect together with {given}: the detector answers the question that flag answers; give one of them")
    elif a.scan_out is not None:
        p.error("--scan-out goes with --scan detect")
    if a.scan is None and a.fields not in ("auto",) + FIELD_ORDERS:
        if a.deinterlacer is not None:
            p.error("--deinterlacer goes with --fields auto, tff or bff, or --scan detect")
        if a.field_rate is not None:
            p.error("--field-rate goes with --fields auto, tff or bff, or --scan detect")
    a.deinterlacer, a.field_rate = a.deinterlacer or DEINTERLACERS[0], a.field_rate or FIELD_RATES[0]
    a.bars = a.bars or "keep"
    a.y4m_in, a.y4m_out = is_y4m(a.input), is_y4m(a.output)
    if not a.y4m_in:
        try:
            resolve_fields(a.fields, None, (25, 1))          # (a Y4M input: once its header is read)
        except ValueError as e:
            p.error(str(e))
    if a.pulldown in (None, "none"):
        if a.pulldown_cycle is not None:
            p.error("--pulldown-cycle goes with --pulldown auto, tff or bff")
    elif a.fields in ("auto",) + FIELD_ORDERS:
        p.error(f"--pulldown {a.pulldown} together with --fields {a.fields}: they are two answers to one question (telecined film, whose "
                f"frames are recovered, or interlaced video, whose fields are interpolated); give one of them")
    a.pulldown_cycle = DEFAULT_CYCLE if a.pulldown_cycle is None else a.pulldown_cycle
    a.combed = None if a.combed == "none" else a.combed
    if a.combed is None:
        if a.comb_threshold is not None or a.comb_pixels is not None:
            p.error("--comb-threshold and --comb-pixels go with --combed yadif or bwdif")
    elif a.scan is None and a.pulldown in (None, "none"):
        p.error(f"--combed {a.combed} goes with --pulldown auto, tff or bff, or --scan detect: it cleans the frames the pulldown removal leaves combed")
    a.comb_threshold = DEFAULT_COMB_THRESHOLD if a.comb_threshold is None else a.comb_threshold
    a.comb_pixels = DEFAULT_COMB_PIXELS if a.comb_pixels is None else a.comb_pixels
    try:
        check_comb_threshold(a.comb_threshold, "--comb-threshold")
        check_comb_pixels(a.comb_pixels, "--comb-pixels")
    except ValueError as e:
        p.error(str(e))
    a.denoise = None if a.denoise == "none" else a.denoise
    if a.denoise is None:
        if a.denoise_radius is not None or a.denoise_strength is not None or a.denoise_chroma_strength is not None:
            p.error("--denoise-radius, --denoise-strength and --denoise-chroma-strength go with --denoise ata")
    elif a.denoise_chroma_strength is not None and not a.y4m_in:
        p.error("--denoise-chroma-strength goes with a Y4M input (PNG frames are RGB: every byte takes --denoise-strength)")
    try:
        a.denoise_radius = check_radius(DEFAULT_RADIUS if a.denoise_radius is None else a.denoise_radius, "--denoise-radius")
        if a.denoise_strength != "auto":
            a.denoise_strength = DEFAULT_STRENGTH if a.denoise_strength is None else parse_strength(a.denoise_strength, "--denoise-strength")
        if a.denoise_chroma_strength is not None:
            a.denoise_chroma_strength = parse_strength(a.denoise_chroma_strength, "--denoise-chroma-strength")
    except ValueError as e:
        p.error(str(e))
    a.spatial_denoise = None if a.spatial_denoise == "none" else a.spatial_denoise
    if a.spatial_denoise is None:
        if any(v is not None for v in (a.spatial_patch, a.spatial_search, a.spatial_strength, a.spatial_chroma_strength)):
            p.error("--spatial-patch, --spatial-search, --spatial-strength and --spatial-chroma-strength go with --spatial-denoise nlm")
    else:
        if a.spatial_chroma_strength is not None and not a.y4m_in:
            p.error("--spatial-chroma-strength goes with a Y4M input (PNG frames are RGB: every channel takes --spatial-strength)")
        try:
            a.spatial_patch = nlm.check_patch(nlm.DEFAULT_PATCH if a.spatial_patch is None else a.spatial_patch, "--spatial-patch")
            a.spatial_search = nlm.check_search(nlm.DEFAULT_SEARCH if a.spatial_search is None else a.spatial_search, "--spatial-search")
            if a.spatial_strength != "auto":
                a.spatial_strength = nlm.check_strength(nlm.DEFAULT_STRENGTH if a.spatial_strength is None else a.spatial_strength, "--spatial-strength")
                nlm.divisor(a.spatial_patch, a.spatial_strength, "--spatial-strength")
            if a.spatial_chroma_strength is not None:
                a.spatial_chroma_strength = nlm.check_strength(a.spatial_chroma_strength, "--spatial-chroma-strength")
                nlm.divisor(a.spatial_patch, a.spatial_chroma_strength, "--spatial-chroma-strength")
        except ValueError as e:
            p.error(str(e))
    autos = [flag for flag, v in (("--denoise-strength", a.denoise_strength), ("--spatial-strength", a.spatial_strength)) if v == "auto"]
    if autos and a.input == "-":
        p.error(f"{autos[0]} auto needs a first pass over the input, which stdin does not allow: measure the noise first "
                f"(savsr_amd.estimate_noise) and give the strength")
    if a.noise_out is not None and not autos:
        p.error("--noise-out goes with --denoise-strength auto or --spatial-strength auto")
    a.deblock = None if a.deblock == "none" else a.deblock
    if a.deblock is None:
        if any(v is not None for v in (a.deblock_block, a.deblock_strength, a.deblock_chroma_strength)):
            p.error("--deblock-block, --deblock-strength and --deblock-chroma-strength go with --deblock weak or strong")
        if any(v is not None for v in (a.deblock_origin, a.deblock_chroma_origin, a.deblock_grid)):
            p.error("--deblock-origin, --deblock-chroma-origin and --deblock-grid go with --deblock weak or strong")
        if a.grid_out is not None:
            p.error("--grid-out goes with --deblock-grid auto")
    else:
        if a.deblock_grid is None and a.grid_out is not None:
            p.error("--grid-out goes with --deblock-grid auto")
        if a.deblock_grid is not None:
            if any(v is not None for v in (a.deblock_block, a.deblock_origin, a.deblock_chroma_origin)):
                p.error("--deblock-grid auto finds what --deblock-block, --deblock-origin and --deblock-chroma-origin say: give one or the other")
            if a.input == "-":
                p.error("--deblock-grid auto needs a first pass over the input, which stdin does not allow: find the grid first "
                        "(savsr_amd.detect_grid) and give --deblock-block / --deblock-origin")
        if a.deblock_chroma_origin is not None and not a.y4m_in:
            p.error("--deblock-chroma-origin goes with a Y4M input (PNG frames are RGB: every channel takes --deblock-origin)")
        if a.deblock_chroma_strength is not None and not a.y4m_in:
            p.error("--deblock-chroma-strength goes with a Y4M input (PNG frames are RGB: every channel takes --deblock-strength)")
        try:
            a.deblock_block = dbk.check_block(dbk.DEFAULT_BLOCK if a.deblock_block is None else a.deblock_block, "--deblock-block")
            a.deblock_strength = (dbk.DEFAULT_STRENGTH if a.deblock_strength is None
                                  else parse_deblock_strength(a.deblock_strength, "--deblock-strength"))
            if a.deblock_chroma_strength is not None:
                a.deblock_chroma_strength = parse_deblock_strength(a.deblock_chroma_strength, "--deblock-chroma-strength")
            a.deblock_origin = (0, 0) if a.deblock_origin is None else parse_deblock_origin(a.deblock_origin, a.deblock_block, "--deblock-origin")
            if a.deblock_chroma_origin is not None:
                a.deblock_chroma_origin = parse_deblock_origin(a.deblock_chroma_origin, a.deblock_block, "--deblock-chroma-origin")
        except ValueError as e:
            p.error(str(e))
    a.dering = None if a.dering == "none" else a.dering
    if a.dering is None:
        if any(v is not None for v in (a.dering_strength, a.dering_chroma_strength, a.dering_damping)):
            p.error("--dering-strength, --dering-chroma-strength and --dering-damping go with --dering cdef")
    else:
        if a.dering_chroma_strength is not None and not a.y4m_in:
            p.error("--dering-chroma-strength goes with a Y4M input (PNG frames are RGB: every channel takes --dering-strength)")
        try:
            a.dering_strength = drg.DEFAULT_STRENGTH if a.dering_strength is None else parse_dering_strength(a.dering_strength, "--dering-strength")
            if a.dering_chroma_strength is not None:
                a.dering_chroma_strength = parse_dering_strength(a.dering_chroma_strength, "--dering-chroma-strength")
            a.dering_damping = drg.check_damping(drg.DEFAULT_DAMPING if a.dering_damping is None else a.dering_damping, "--dering-damping")
        except ValueError as e:
            p.error(str(e))
    try:
        check_cycle(a.pulldown_cycle, "--pulldown-cycle")
        if not a.y4m_in:
            resolve_pulldown(a.pulldown, None, (25, 1), a.pulldown_cycle)          # (a Y4M input: once its header is read)
    except ValueError as e:
        p.error(str(e))
    if a.fps is not None and (a.y4m_in or not a.y4m_out):
        p.error("--fps goes with a PNG folder in and Y4M out (a Y4M input carries its frame rate, PNGs have none)")
    if a.colour is not None and not a.y4m_in:
        p.error("--colour goes with a Y4M input (PNG frames are RGB)")
    if a.out_colour is not None and not a.y4m_out:
        p.error("--out-colour goes with a Y4M output (PNG frames are RGB)")
    if a.out_depth is not None and not a.y4m_out:
        p.error("--out-depth goes with a Y4M output (PNG frames are 8-bit RGB)")
    if a.out_chroma is not None and not a.y4m_out:
        p.error("--out-chroma goes with a Y4M output (PNG frames are RGB)")
    if a.siting is not None and not a.y4m_in:
        p.error("--siting goes with a Y4M input (PNG frames are RGB)")
    if a.out_siting is not None and not a.y4m_out:
        p.error("--out-siting goes with a Y4M output (PNG frames are RGB)")
    a.chroma_filter = None if a.chroma_filter == "none" else a.chroma_filter
    a.dither = None if a.dither == "none" else a.dither
    if a.chroma_filter is not None and not (a.y4m_in and a.y4m_out):
        p.error("--chroma-filter goes with a Y4M input and a Y4M output (the chroma planes come from the one and go to the other)")
    a.siting = a.siting or "none"
    a.out_siting = a.out_siting or "none"
    a.out_depth = None if a.out_depth in (None, "same") else int(a.out_depth)          # (None: the input's)
    a.out_chroma = None if a.out_chroma in (None, "same") else a.out_chroma            # (None: the input's)
    a.colour_flags = a.colour is not None or a.out_colour is not None       # (either given: the output is tagged, the summary names them)
    a.colour = a.colour or "bt601"
    a.out_colour = a.out_colour or "same"
    from .y4m import parse_fps
    try:
        a.fps = parse_fps(a.fps) if a.fps is not None else (25, 1)
    except ValueError as e:
        p.error(f"--fps: {e}")
    return a


def list_frames(folder: str) -> List[str]:
    from .io import scandir
    if not os.path.isdir(folder):
        raise SystemExit(f"input folder {folder!r} does not exist")
    paths = sorted(scandir(folder, suffix=".png", full_path=True))
    if not paths:
        raise SystemExit(f"no .png frames in {folder!r}")
    return paths


def load_net(a: argparse.Namespace):
    """The network as models.py builds it from a YAML (network_g, path.*), or SAVSR() from a bare checkpoint."""
    from . import io as sio
    from .archs import build_network
    from .archs.savsr_arch import SAVSR
    if a.opt is not None:
        from .options import yaml_load
        opt = yaml_load(a.opt)
        net = build_network(opt["network_g"])
        path = opt.get("path") or {}
        if path.get("pretrain_network_g") is not None:
            sio.load_network(net, path["pretrain_network_g"], path.get("strict_load_g", True), path.get("param_key_g", "params"))
    else:
        net = SAVSR()
        sio.load_network(net, a.checkpoint, True, "params")
    if net.cfg["num_in_ch"] == 1 and a.y4m_in and a.y4m_out:
        return net.eval()          # (a luma-only checkpoint: main() asks for --chroma-filter or a grey-scale input once the header is read)
    if a.chroma_filter is not None:
        raise SystemExit(f"--chroma-filter = {a.chroma_filter!r} with num_in_ch = {net.cfg['num_in_ch']}: chroma goes through such a network")
    if net.cfg["num_in_ch"] != 3:
        raise SystemExit(f"num_in_ch = {net.cfg['num_in_ch']}: the CLI decodes RGB frames; run such a checkpoint through SAVSR.upscale_video")
    return net.eval()


class Y4MSink:
    """SR frames [k, i420_bytes] on the GPU -> the Y4M writer: an asynchronous copy into one of PINNED_BUFFERS pinned host buffers on
    the caller's stream, then one writer thread that waits for the copy's event and writes the frames in order.  emit() blocks only
    when every buffer is still waiting to be written."""

    def __init__(self, writer, capacity: int):
        self.writer, self.capacity = writer, max(1, capacity)
        self.todo: "queue.Queue" = queue.Queue()
        self.free: "queue.Queue" = queue.Queue()
        self.made = 0
        self.error: Optional[BaseException] = None
        self.thread = threading.Thread(target=self._loop, name="savsr-upscale-y4m", daemon=True)
        self.thread.start()

    def _buffer(self, k: int):
        import torch
        buf = None
        if self.made < PINNED_BUFFERS:
            self.made += 1
        else:
            buf = self.free.get()
        if buf is None or buf.shape[0] < k:
            buf = torch.empty(max(k, self.capacity), self.writer.frame_bytes, dtype=torch.uint8).pin_memory()
        return buf

    def emit(self, sr) -> int:
        import torch
        k = int(sr.shape[0])
        if k:
            buf = self._buffer(k)
            buf[:k].copy_(sr, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            self.todo.put((buf, k, done))
        return k

    def _loop(self) -> None:
        while True:
            item = self.todo.get()
            if item is None:
                return
            buf, k, done = item
            try:
                if self.error is None:
                    done.synchronize()
                    self.writer.write(buf[:k].numpy())
            except BaseException as e:          # (kept for close(); the buffers keep circulating so that emit() never hangs)
                self.error = e
            self.free.put(buf)

    def close(self) -> None:
        self.todo.put(None)
        self.thread.join()
        if self.error is None:
            self.writer.f.flush()
        else:
            raise self.error


class PngSink:
    """SR frames [k, H, W, 3] uint8 on the GPU -> PNG files, encoded on a pool of writer threads."""

    def __init__(self, folder: str, names: Optional[List[str]], n_writers: int):
        os.makedirs(folder, exist_ok=True)
        self.folder, self.names, self.count = folder, names, 0
        self.pool = ThreadPoolExecutor(max_workers=n_writers, thread_name_prefix="savsr-upscale-png")
        self.pending: list = []

    @staticmethod
    def _save(img, path: str) -> None:
        from PIL import Image
        Image.fromarray(img).save(path)

    def emit(self, sr) -> int:
        host = sr.cpu().numpy()
        for j in range(host.shape[0]):
            name = self.names[self.count] if self.names is not None else f"{self.count:08d}.png"
            self.pending.append(self.pool.submit(self._save, host[j], os.path.join(self.folder, name)))
            self.count += 1
        while len(self.pending) > 4 * MAX_WRITERS:          # bound the queue of encoded-but-unwritten frames
            self.pending.pop(0).result()
        return host.shape[0]

    def close(self) -> None:
        for f in self.pending:
            f.result()
        self.pool.shutdown()


def written_lr(h, w, rect, bars: str):
    """The LR size behind the frames actually written: the rect's with --bars drop, the frame's otherwise.  The output's size, its pixel
    aspect and its `auto` colour space follow from it."""
    return (h, w) if rect is None or bars == "keep" else (rect[2], rect[3])


def denoise_kwargs(a: argparse.Namespace) -> dict:
    """--denoise and its options as the keyword arguments of VideoUpscaler; nothing without --denoise."""
    if a.denoise is None:
        return {}
    return dict(denoise=a.denoise, denoise_radius=a.denoise_radius, denoise_strength=a.denoise_strength,
                denoise_chroma_strength=a.denoise_chroma_strength)


def spatial_kwargs(a: argparse.Namespace) -> dict:
    """--spatial-denoise and its options as the keyword arguments of VideoUpscaler; nothing without --spatial-denoise."""
    if a.spatial_denoise is None:
        return {}
    return dict(spatial_denoise=a.spatial_denoise, spatial_patch=a.spatial_patch, spatial_search=a.spatial_search,
                spatial_strength=a.spatial_strength, spatial_chroma_strength=a.spatial_chroma_strength)


def deblock_kwargs(a: argparse.Namespace) -> dict:
    """--deblock and its options as the keyword arguments of VideoUpscaler; nothing without --deblock."""
    if a.deblock is None:
        return {}
    kw = dict(deblock=a.deblock, deblock_block=a.deblock_block, deblock_strength=a.deblock_strength,
              deblock_chroma_strength=a.deblock_chroma_strength)
    if tuple(a.deblock_origin) != (0, 0) or a.deblock_chroma_origin is not None:          # (an origin at its default: the call as it was)
        kw.update(deblock_origin=a.deblock_origin, deblock_chroma_origin=a.deblock_chroma_origin)
    return kw


def dering_kwargs(a: argparse.Namespace) -> dict:
    """--dering and its options as the keyword arguments of VideoUpscaler; nothing without --dering."""
    if a.dering is None:
        return {}
    return dict(dering=a.dering, dering_strength=a.dering_strength, dering_chroma_strength=a.dering_chroma_strength,
                dering_damping=a.dering_damping)


def detect_grid_pass(a: argparse.Namespace, chunks, fmt_in: str, size, depth: int, dev, fieldwise: bool):
    """--deblock-grid auto's first pass: savsr_amd.grid_stats over the input in --chunk-sized pieces, summed on the device (one copy of 64
    integers at the end), then grid.verdict_from_stats.  It reads the frames the deblocker will read -- as decoded, field-wise exactly
    when the stage will run field-wise -- so it comes after --scan detect's pass, whose verdict says which, and in front of --crop
    auto's, which reads the filtered frames.  chunks: the PNG folder's chunk iterator; None: the .y4m file named by --input, read
    through a reader of its own."""
    import torch

    from .grid import frame_pairs, verdict_from_stats
    from .prepass import grid_stats
    from .y4m import Y4MReader
    from .yuv import CHROMAS
    f = None
    table, pairs = None, None
    try:
        if chunks is None:
            f = open(a.input, "rb")
            chunks = (torch.from_numpy(c) for c in Y4MReader(f, high_depth=True, layouts=CHROMAS, mono=True).chunks(a.chunk))
        with torch.cuda.device(dev):
            for chunk in chunks:
                if not int(chunk.shape[0]):
                    continue
                part = grid_stats(chunk.to(dev), fmt_in, size, depth, fieldwise).sum(0)
                more = int(chunk.shape[0]) * frame_pairs(tuple(chunk.shape), fmt_in, size, depth, fieldwise)
                table, pairs = (part, more) if table is None else (table + part, pairs + more)
    except ValueError as e:
        raise SystemExit(f"--deblock-grid auto: {e}") from None
    finally:
        if f is not None:
            f.close()
    if table is None:
        raise SystemExit("the video has no frames")
    return verdict_from_stats(table.cpu().numpy(), pairs, fieldwise)


def front_frames(a: argparse.Namespace, chunks, fmt_in: str, size, depth: int, dev, order: Optional[str] = None, film: Optional[str] = None,
                 denoise: bool = True):
    """The front chain of a first pass, as the second pass will run it: the input in --chunk-sized pieces through --deblock, --dering
    (field by field with `order` / `film`), the --fields / --pulldown stage (a prepass.FieldSplitter / PulldownRemover of this pass's
    own) and, with `denoise`, --denoise (a prepass.TemporalDenoiser of its own); yields the chunks of progressive frames that come out,
    on the device.  chunks: the PNG folder's chunk iterator; None: the .y4m file named by --input, read through a reader of its own."""
    import torch

    from .frames import detector_side
    from .prepass import deblock_video, dering_video, make_denoiser, make_stage
    from .y4m import Y4MReader
    from .yuv import CHROMAS
    f = None
    how = (a.deinterlacer, a.field_rate) if order is not None else ()          # (they say how --fields is carried out, and nothing else)
    comb = dict(combed=a.combed, comb_threshold=a.comb_threshold, comb_pixels=a.comb_pixels) if film is not None and a.combed is not None else {}
    split = make_stage(order, film, a.pulldown_cycle, *detector_side(fmt_in, size, depth), *how, **comb)
    noise = None
    if denoise and a.denoise is not None:          # (None also where --denoise-strength auto found no noise: its options then say nothing)
        noise = make_denoiser(a.denoise, a.denoise_radius, a.denoise_strength, a.denoise_chroma_strength, *detector_side(fmt_in, size, depth))

    def behind(frames, final: bool = False):          # the chunks behind the denoiser: what it lets go of
        if frames is None or not int(frames.shape[0]):
            return
        if noise is not None and not final:
            frames = noise.push(frames)
        if int(frames.shape[0]):
            yield frames

    try:
        if chunks is None:
            f = open(a.input, "rb")
            chunks = (torch.from_numpy(c) for c in Y4MReader(f, high_depth=True, layouts=CHROMAS, mono=True).chunks(a.chunk))
        with torch.cuda.device(dev):
            for chunk in chunks:
                chunk = chunk.to(dev)
                if a.deblock is not None:
                    chunk = deblock_video(chunk, fmt_in, size, depth, a.deblock_block, a.deblock, a.deblock_strength, a.deblock_chroma_strength,
                                          order is not None or film is not None, a.deblock_origin, a.deblock_chroma_origin)
                if a.dering is not None:
                    chunk = dering_video(chunk, fmt_in, size, depth, a.dering_strength, a.dering_chroma_strength, a.dering_damping,
                                         order is not None or film is not None)
                yield from behind(chunk if split is None else split.push(chunk))
            yield from behind(None if split is None else split.finish())
            yield from behind(None if noise is None else noise.finish(), True)
    finally:
        if f is not None:
            f.close()


def detect_crop(a: argparse.Namespace, chunks, fmt_in: str, size, depth: int, dev, order: Optional[str] = None, film: Optional[str] = None):
    """--crop auto's first pass: savsr_amd.line_sums over the input in --chunk-sized pieces with a running maximum on the device, then
    cropdetect's rule and the alignment to the input layout's chroma block.  The sums are taken behind `front_frames`: on the frames the
    second pass will crop -- filtered by --deblock / --dering, deinterlaced with `order` (--fields' field order) or recovered with `film`
    (--pulldown's), denoised by --denoise, as upscale_video's crop="auto" takes them."""
    import torch

    from . import active
    from .frames import layout_of
    from .prepass import line_sums
    top = None
    with torch.cuda.device(dev):
        for frames in front_frames(a, chunks, fmt_in, size, depth, dev, order, film):
            c = 1 if size else int(frames.shape[3])
            h, w = size if size else (int(frames.shape[1]), int(frames.shape[2]))
            rows, cols = line_sums(frames, fmt_in, size, depth)
            now = torch.cat([rows.amax(0), cols.amax(0)])
            top = now if top is None else torch.maximum(top, now)
    if top is None:
        raise SystemExit("the video has no frames")
    top = top.cpu().tolist()
    s_row, s_col = active.line_samples(h, w, c)
    return active.align_rect(active.active_rect(top[:h], top[h:], s_row, s_col, a.crop_limit), layout_of(fmt_in) if size else None)


def describe_noise(verdict) -> str:
    """A NoiseVerdict in a few words for stderr: sigma per class in 8-bit code units, the cells behind it and the flat ones."""
    def one(s):
        return "unknown (too few cells)" if s is None else f"{float(s):.3f}"
    text = f"sigma {one(verdict.sigma)} from {verdict.cells[0]} cells ({verdict.flat[0]} flat)"
    if verdict.cells[1] or verdict.flat[1]:
        text += f", chroma sigma {one(verdict.chroma_sigma)} from {verdict.cells[1]} cells ({verdict.flat[1]} flat)"
    return text


def noise_pass(a: argparse.Namespace, chunks, fmt_in: str, size, depth: int, dev, order: Optional[str] = None, film: Optional[str] = None,
               rect=None, spatial: bool = False):
    """The first pass of --denoise-strength auto (spatial False) or --spatial-strength auto (spatial True): savsr_amd.noise_stats over
    the frames its stage will read, summed on the device (one copy of 1024 integers at the end), then noise.verdict_from_stats.  The
    temporal one measures behind `front_frames` without the denoiser; the spatial one behind the denoiser, at the strength just found,
    and behind the crop to `rect`, so it sees the noise that is left inside the picture."""
    import torch

    from .active import check_rect
    from .frames import detector_side, layout_of
    from .noise import verdict_from_stats
    from .prepass import _crop_device, noise_stats
    side, hw = detector_side(fmt_in, size, depth)
    table = None
    try:
        with torch.cuda.device(dev):
            for frames in front_frames(a, chunks, fmt_in, size, depth, dev, order, film, denoise=spatial):
                at = size
                if spatial and rect is not None:
                    h, w = size if size else (int(frames.shape[1]), int(frames.shape[2]))
                    rect = check_rect(rect, h, w, layout_of(fmt_in) if size else None)
                    if tuple(rect) != (0, 0, h, w):
                        frames, at = _crop_device(frames, rect, side, (h, w)), ((rect[2], rect[3]) if size else None)
                part = noise_stats(frames, fmt_in, at, depth).sum(0)
                table = part if table is None else table + part
    except ValueError as e:
        raise SystemExit(f"--{'spatial' if spatial else 'denoise'}-strength auto: {e}") from None
    if table is None:
        raise SystemExit("the video has no frames")
    return verdict_from_stats(table.cpu().numpy())


def detect_scan_pass(a: argparse.Namespace, chunks, fmt_in: str, size, depth: int, dev):
    """--scan detect's first pass: a prepass.ScanStats over the input in --chunk-sized pieces (the field statistics on the GPU, one row per
    frame brought to the host), then scan.verdict_from_stats.  chunks: the PNG folder's chunk iterator; None: the .y4m file named by
    --input, read through a reader of its own."""
    import numpy as np
    import torch

    from .frames import detector_side
    from .prepass import ScanStats
    from .scan import STAT_COLUMNS, verdict_from_stats
    from .y4m import Y4MReader
    from .yuv import CHROMAS
    f = None
    acc = ScanStats(*detector_side(fmt_in, size, depth))
    rows = []
    try:
        if chunks is None:
            f = open(a.input, "rb")
            chunks = (torch.from_numpy(c) for c in Y4MReader(f, high_depth=True, layouts=CHROMAS, mono=True).chunks(a.chunk))
        with torch.cuda.device(dev):
            for chunk in chunks:
                rows.append(acc.push(chunk.to(dev)).cpu().numpy())
            last = acc.finish()
            if last is not None:
                rows.append(last.cpu().numpy())
    except ValueError as e:          # (frames the detector does not take: one row)
        raise SystemExit(f"--scan detect: {e}") from None
    finally:
        if f is not None:
            f.close()
    if not rows:
        raise SystemExit("the video has no frames")
    return verdict_from_stats(np.concatenate(rows, 0).reshape(-1, STAT_COLUMNS))


def main(argv: Optional[List[str]] = None) -> int:
    a = parse_args(argv)
    paths = None if a.y4m_in else list_frames(a.input)
    import numpy as np
    import torch

    from .packing import get_hw
    from .utils.host import effective_cpus
    from .video import VideoUpscaler, check_length
    from .y4m import Y4MReader, Y4MWriter, scaled_aspect
    from .yuv import CHROMAS, FORMAT_OF, LUMA_FORMAT, MONO, is_full_range

    net = load_net(a)
    net.set_precision(a.precision)
    net.set_self_ensemble(a.self_ensemble)
    per_file = 1 if a.field_rate == "same" else 2                 # (--fields: two frames per file; --field-rate same: one)
    n_png = None if paths is None else len(paths) * (per_file if a.fields in FIELD_ORDERS else 1)
    if paths is not None and a.pulldown in FIELD_ORDERS:
        n_png -= n_png // a.pulldown_cycle                        # (--pulldown: one frame of every cycle is dropped)

    def check_png_count(n):                                       # (a Y4M stream's length: at its end)
        if a.cuts is None:
            check_length(n, net.num_frame, a.padding)
        elif a.cuts != "auto":
            from .scenes import check_cuts
            check_cuts(a.cuts, n)
    if paths is not None and a.scan is None:
        check_png_count(n_png)                                    # (before the GPU is touched; --scan detect: once the verdict is known)
    fin = fout = None
    try:
        if a.y4m_in:
            if a.input != "-" and not os.path.isfile(a.input):
                raise SystemExit(f"input file {a.input!r} does not exist")
            fin = sys.stdin.buffer if a.input == "-" else open(a.input, "rb")
            reader = Y4MReader(fin, high_depth=True, layouts=CHROMAS, mono=True)
            h, w, depth, chroma = reader.height, reader.width, reader.depth, reader.chroma
            nch = net.cfg["num_in_ch"]
            if chroma == MONO and nch != 1:
                raise SystemExit(f"the input is grey-scale (C{reader.colorspace}): it needs a luma-only checkpoint (num_in_ch = 1), this one has "
                                 f"num_in_ch = {nch}")
            if chroma == MONO and a.out_chroma is not None:
                raise SystemExit(f"--out-chroma = {a.out_chroma!r} with a grey-scale input: it has no chroma planes; the output is grey-scale")
            if nch == 1 and chroma != MONO and a.chroma_filter is None:
                raise SystemExit("num_in_ch = 1 with a colour Y4M input: give --chroma-filter bicubic (Y through the network, Cb / Cr resampled)")
            fps, interlace, aspect, in_range = reader.fps, reader.interlace, reader.aspect, reader.colour_range
            tag_siting = reader.siting
            chunks = (torch.from_numpy(c) for c in reader.chunks(a.chunk))
        else:
            from .io import FrameStore
            store = FrameStore()
            h = w = None
            depth, chroma, tag_siting = 8, "420", None
            if a.y4m_out:                           # (the Y4M header needs the SR size before the first frame: the PNG's header gives it)
                from PIL import Image
                with Image.open(paths[0]) as im:
                    w, h = im.size
            fps, interlace, aspect, in_range = a.fps, "p", (0, 0), None

            def png_chunks():
                store.request(paths)
                for c0 in range(0, len(paths), a.chunk):
                    yield torch.from_numpy(np.stack([store.host(p) for p in paths[c0:c0 + a.chunk]], 0))
            chunks = png_chunks()
        fmt_of = dict(FORMAT_OF, **{MONO: LUMA_FORMAT})
        fmt_in = fmt_of[chroma] if a.y4m_in else "rgb"
        verdict = None
        if a.scan is not None:                      # the first pass of --scan detect: the content says what --fields / --pulldown would have said
            from .scan import tag_note
            dev = torch.device(a.device)
            net = net.to(dev)
            verdict = detect_scan_pass(a, chunks if paths is not None else None, fmt_in, (h, w) if a.y4m_in else None, depth, dev)
            if paths is not None:
                chunks = png_chunks()
            found = verdict.kwargs()
            a.pulldown = found.get("pulldown")
            a.fields = found.get("fields", "progressive" if verdict.scan == "progressive" else None)
            print(f"--scan detect: {verdict.describe()}: {verdict.flag() or 'no --fields, no --pulldown'}", file=sys.stderr, flush=True)
            note = tag_note(verdict, interlace if a.y4m_in else None)
            if note is not None:
                print(note, file=sys.stderr, flush=True)
            if a.scan_out is not None:
                import json
                with open(a.scan_out, "w") as f:
                    json.dump(verdict.as_json(), f)
                    f.write("\n")
            if paths is not None:
                n_png = len(paths) * (per_file if a.fields in FIELD_ORDERS else 1)
                if a.pulldown in FIELD_ORDERS:
                    n_png -= n_png // a.pulldown_cycle
                try:
                    check_png_count(n_png)
                except ValueError as e:
                    raise SystemExit(str(e)) from None
        try:                                        # --pulldown and the input's I tag: the field order, the output's I tag and frame rate
            film, film_tag, film_fps, film_note = resolve_pulldown(a.pulldown, interlace if a.y4m_in else None, fps, a.pulldown_cycle)
        except ValueError as e:
            raise SystemExit(str(e)) from None
        if film_note is not None:
            print(film_note, file=sys.stderr, flush=True)
        if film is not None:                        # (the fields are matched, not interpolated: --fields has nothing left to say)
            order, interlace, fps = None, film_tag, film_fps
        else:
            try:                                    # --fields and the input's I tag: the field order, the output's I tag and frame rate
                order, interlace, fps, note = resolve_fields(a.fields, interlace if a.y4m_in else None, fps, a.field_rate)
            except ValueError as e:
                raise SystemExit(str(e)) from None
            if note is not None:
                print(note, file=sys.stderr, flush=True)
        dev = torch.device(a.device)
        net = net.to(dev)
        fieldwise = order is not None or film is not None
        if a.deblock is not None and a.deblock_grid is not None:          # the grid's pass: behind the scan's, whose verdict it needs, in front of the crop's
            found = detect_grid_pass(a, chunks if paths is not None else None, fmt_in, (h, w) if a.y4m_in else None, depth, dev, fieldwise)
            if paths is not None:
                chunks = png_chunks()
            if a.grid_out is not None:
                import json
                with open(a.grid_out, "w") as f:
                    json.dump(found.as_json(), f)
                    f.write("\n")
            kw = found.kwargs()
            if not kw:
                print("--deblock-grid auto: no grid found: --deblock none (the rule is not validated on footage)", file=sys.stderr, flush=True)
                a.deblock = None
            else:
                a.deblock_block, a.deblock_origin = kw["deblock_block"], kw["deblock_origin"]
                a.deblock_chroma_origin = kw.get("deblock_chroma_origin")
                a.deblock_chroma_strength = kw.get("deblock_chroma_strength", a.deblock_chroma_strength)
                flags = f"--deblock-block {a.deblock_block} --deblock-origin {a.deblock_origin[0]},{a.deblock_origin[1]}"
                if a.deblock_chroma_origin is not None:
                    flags += f" --deblock-chroma-origin {a.deblock_chroma_origin[0]},{a.deblock_chroma_origin[1]}"
                if "deblock_chroma_strength" in kw:
                    flags += " --deblock-chroma-strength 0,0 (no chroma grid of that block: the chroma planes are left alone)"
                print(f"--deblock-grid auto: block {a.deblock_block} at origin {a.deblock_origin[0]},{a.deblock_origin[1]}"
                      f"{' (field-wise)' if fieldwise else ''}: {flags} (the rule is not validated on footage)", file=sys.stderr, flush=True)
        if a.deblock is not None:
            try:          # (an odd Y on a field-wise run, a subsampled input without a chroma origin: known only now)
                dbk.check_origins(a.deblock_origin, a.deblock_chroma_origin, a.deblock_block, fieldwise,
                                  chroma if a.y4m_in and chroma != MONO else None, "--deblock-")
            except ValueError as e:
                raise SystemExit(str(e)) from None
        noise_report = {}                           # what --noise-out writes: the verdict and the chosen flags of each measuring point
        if a.denoise is not None and a.denoise_strength == "auto":          # the temporal noise's pass: behind the grid's, in front of the crop's
            found = noise_pass(a, chunks if paths is not None else None, fmt_in, (h, w) if a.y4m_in else None, depth, dev, order, film)
            if paths is not None:
                chunks = png_chunks()
            kw = found.denoise_kwargs()
            if not kw:
                flags, a.denoise = "--denoise none", None
            else:
                a.denoise_strength = kw["denoise_strength"]
                if a.denoise_chroma_strength is None and a.y4m_in:
                    a.denoise_chroma_strength = kw.get("denoise_chroma_strength")
                flags = f"--denoise {a.denoise} --denoise-strength {a.denoise_strength[0]},{a.denoise_strength[1]}"
                if a.denoise_chroma_strength is not None:
                    flags += f" --denoise-chroma-strength {a.denoise_chroma_strength[0]},{a.denoise_chroma_strength[1]}"
            print(f"--denoise-strength auto: {describe_noise(found)}: {flags} (the measure is not validated on footage)", file=sys.stderr, flush=True)
            noise_report["denoise"] = dict(found.as_json(), flags=flags)
        rect = a.crop
        if rect == "auto":                          # the first pass: line sums chunk by chunk, a running maximum on the device
            rect = detect_crop(a, chunks if paths is not None else None, fmt_in, (h, w) if a.y4m_in else None, depth, dev, order, film)
            if paths is not None:
                chunks = png_chunks()
            print(f"--crop auto: active picture {rect[2]} x {rect[3]} at ({rect[0]}, {rect[1]}): --crop {','.join(str(v) for v in rect)}",
                  file=sys.stderr, flush=True)
        elif rect is not None and h is not None:
            from .active import check_rect
            from .video import layout_of
            try:
                rect = check_rect(rect, h, w, layout_of(fmt_in) if a.y4m_in else None)
            except ValueError as e:
                raise SystemExit(f"--crop: {e}") from None
        if a.spatial_denoise is not None and a.spatial_strength == "auto":          # the spatial noise's pass: behind --denoise as found and the crop
            found = noise_pass(a, chunks if paths is not None else None, fmt_in, (h, w) if a.y4m_in else None, depth, dev, order, film, rect, True)
            if paths is not None:
                chunks = png_chunks()
            kw = found.spatial_kwargs()
            if not kw:
                flags, a.spatial_denoise = "--spatial-denoise none", None
            else:
                a.spatial_strength = kw["spatial_strength"]
                if a.spatial_chroma_strength is None and a.y4m_in:
                    a.spatial_chroma_strength = kw.get("spatial_chroma_strength")
                flags = f"--spatial-denoise {a.spatial_denoise} --spatial-strength {a.spatial_strength:g}"
                if a.spatial_chroma_strength is not None:
                    flags += f" --spatial-chroma-strength {a.spatial_chroma_strength:g}"
            print(f"--spatial-strength auto: {describe_noise(found)}: {flags} (the measure is not validated on footage)", file=sys.stderr, flush=True)
            noise_report["spatial"] = dict(found.as_json(), flags=flags)
        if a.noise_out is not None:
            import json
            with open(a.noise_out, "w") as f:
                json.dump(noise_report, f)
                f.write("\n")
        lr = written_lr(h, w, rect, a.bars)
        hr = get_hw(lr[0], lr[1], a.scale) if a.y4m_out else None
        colour, out_colour = resolve_colours(a.colour, a.out_colour, (h, w) if a.y4m_in else None, hr, in_range)
        out_depth = (depth if a.out_depth is None else a.out_depth) if a.y4m_out else None
        out_chroma = (chroma if a.out_chroma is None else a.out_chroma) if a.y4m_out else None
        fmt_out = fmt_of[out_chroma] if a.y4m_out else "uint8"
        from .video import check_depths
        try:                                        # (before the output is opened: a full-range colour with 10 / 12 bits is refused)
            check_depths(depth, out_depth, fmt_in, fmt_out, colour or "bt601", out_colour)
        except ValueError as e:
            raise SystemExit(f"--colour / --out-colour / --out-depth: {e}") from None
        try:
            siting, out_siting = resolve_sitings(a.siting, a.out_siting, tag_siting, chroma if a.y4m_in and chroma != MONO else None,
                                                 None if out_chroma == MONO else out_chroma)
        except ValueError as e:
            raise SystemExit(f"--siting / --out-siting: {e}") from None
        if a.siting == "auto":
            print(f"--siting auto: C{reader.colorspace} -> {siting or 'none'}", file=sys.stderr, flush=True)
        if a.y4m_out:
            H, W = hr
            fout = sys.stdout.buffer if a.output == "-" else open(a.output, "wb")
            full = is_full_range(out_colour)
            tag = ("full" if full else "limited") if (full or a.colour_flags) else None
            sink = Y4MSink(Y4MWriter(fout, W, H, fps, interlace, scaled_aspect(aspect, lr, (H, W)), tag, depth=out_depth, chroma=out_chroma,
                                     siting=out_siting),
                           a.chunk + net.num_frame)
        else:
            sink = PngSink(a.output, None if paths is None or order is not None or film is not None else [os.path.basename(p) for p in paths],
                           a.writers or max(1, min(MAX_WRITERS, effective_cpus())))
        t0 = time.perf_counter()
        up = VideoUpscaler(net, a.scale, a.padding, out=fmt_out, pixel_format=fmt_in,
                           size=(h, w) if a.y4m_in else None, cuts=a.cuts, scene_threshold=a.scene_threshold,
                           colour="bt601" if chroma == MONO else colour or "bt601",          # (grey-scale frames carry no colour space)
                           out_colour=None if out_chroma == MONO else out_colour, depth=depth, out_depth=out_depth, siting=siting, out_siting=out_siting,
                           chroma_filter=a.chroma_filter, crop=rect, bars=a.bars, fields=order, pulldown=film, pulldown_cycle=a.pulldown_cycle,
                           dither=a.dither, **(dict(deinterlacer=a.deinterlacer, field_rate=a.field_rate) if order is not None else {}),
                           # (--combed with --scan detect says how a telecine verdict is carried out: ignored for the other verdicts)
                           **(dict(combed=a.combed, comb_threshold=a.comb_threshold, comb_pixels=a.comb_pixels)
                              if film is not None and a.combed is not None else {}),
                           **denoise_kwargs(a), **spatial_kwargs(a), **deblock_kwargs(a), **dering_kwargs(a))
        if a.deblock is not None:
            cs = a.deblock_chroma_strength or a.deblock_strength
            at = "" if a.deblock_origin == (0, 0) and a.deblock_chroma_origin is None else (
                f" at origin {a.deblock_origin[0]},{a.deblock_origin[1]}"
                + ("" if a.deblock_chroma_origin is None else f" (chroma {a.deblock_chroma_origin[0]},{a.deblock_chroma_origin[1]})"))
            print(f"--deblock {a.deblock}: block {a.deblock_block}{at}, strength {a.deblock_strength[0]},{a.deblock_strength[1]}"
                  + (f", chroma strength {cs[0]},{cs[1]}" if a.y4m_in else "") + " (8-bit code units; not validated on footage), "
                  + ("field-wise (the fields as planes of their own)" if order is not None or film is not None else "progressive"),
                  file=sys.stderr, flush=True)
        if a.dering is not None:
            cs = a.dering_chroma_strength or a.dering_strength
            print(f"--dering {a.dering}: strength {a.dering_strength[0]},{a.dering_strength[1]}"
                  + (f", chroma strength {cs[0]},{cs[1]}" if a.y4m_in else "") + f", damping {a.dering_damping} (8-bit code units; not validated on "
                  + "footage), " + ("field-wise (the fields as planes of their own)" if order is not None or film is not None else "progressive"),
                  file=sys.stderr, flush=True)
        if a.spatial_denoise is not None:
            ch = a.spatial_strength if a.spatial_chroma_strength is None else a.spatial_chroma_strength
            print(f"--spatial-denoise {a.spatial_denoise}: patch {a.spatial_patch} ({2 * a.spatial_patch + 1} x {2 * a.spatial_patch + 1}), search "
                  f"{a.spatial_search} ({2 * a.spatial_search + 1} x {2 * a.spatial_search + 1}), strength {a.spatial_strength:g}"
                  + (f", chroma strength {ch:g}" if a.y4m_in else "") + " (8-bit code units; not validated on footage)", file=sys.stderr, flush=True)
        if a.denoise is not None:
            cs = a.denoise_chroma_strength or a.denoise_strength
            print(f"--denoise {a.denoise}: radius {a.denoise_radius} ({2 * a.denoise_radius + 1} frames), strength {a.denoise_strength[0]},"
                  f"{a.denoise_strength[1]}" + (f", chroma strength {cs[0]},{cs[1]}" if a.y4m_in else "")
                  + " (8-bit code units; not validated on footage)", file=sys.stderr, flush=True)
        done = 0
        try:
            for chunk in chunks:
                done += sink.emit(up.push(chunk))
            done += sink.emit(up.finish())
        finally:
            sink.close()
        dt = time.perf_counter() - t0
    finally:
        for f, std in ((fin, sys.stdin.buffer), (fout, sys.stdout.buffer)):
            if f is not None and f is not std:
                f.close()
    scenes = ""
    if a.cuts is not None:
        scenes = f", {len(up.cuts) + 1} scenes"
        if a.cuts_out is not None:
            with open(a.cuts_out, "w") as f:
                f.writelines(f"{k}\n" for k in up.cuts)
    if a.colour_flags:
        scenes += f", colour {colour or 'rgb'} -> {out_colour or 'rgb'}"
    if depth != 8 or (out_depth or 8) != 8:
        scenes += f", {depth} -> {out_depth or 8} bits"
    if chroma != "420" or (out_chroma or "420") != "420":
        scenes += f", chroma {chroma if a.y4m_in else 'rgb'} -> {out_chroma or 'rgb'}"
    if siting is not None or out_siting is not None:
        scenes += f", siting {siting or 'none'} -> {out_siting or 'none'}"
    if a.dither is not None:
        scenes += f", dither {a.dither}"
    if order is not None:
        scenes += f", fields {order}" + (f" ({a.deinterlacer}, {a.field_rate} rate)" if (a.deinterlacer, a.field_rate) != ("yadif", "double") else "")
    if verdict is not None:
        scenes += f", scan {verdict.describe()}"
    if film is not None:
        info = up.pulldown_info
        scenes += (f", pulldown {film}: {len(info['matches'])} frames in, {len(info['kept'])} out, {info['matches'].count(-1)} matched from "
                   f"their predecessor")
        if "combed" in info:
            print(f"--combed {a.combed}: {len(info['combed'])} of {len(info['matches'])} woven frames were combed and deinterlaced",
                  file=sys.stderr, flush=True)
    print(f"upscaled {done} frames in {dt:.2f} s: {done / dt:.2f} frames/s{scenes}", file=sys.stderr if a.output == "-" else sys.stdout, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
