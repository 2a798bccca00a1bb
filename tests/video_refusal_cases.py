"""Case table of the refusal census of the video boundary, shared by tools/video_refusals.py (the whole grid) and
tests/test_video_refusals.py (a fixed subsample against tests/golden/video_refusals.json).

A case is one choice of every format argument of SAVSR.upscale_video / VideoUpscaler on a CPU network (num_in_ch = 3 or 1).  Its record
is what the two entry points answer: (exception type, message) each, or "constructed" for a VideoUpscaler that accepts its arguments.  A
valid upscale_video call on a CPU network ends at the "runs on an AMD GPU only" RuntimeError, which is its record: every check of the
arguments has passed by then.  Which check speaks first when several would refuse is part of the record.

Case k < GRID_CASES is position k of the product over NCH and AXES in their order here (the last axis fastest); the cases behind
them are TENSOR_CASES, wrong frames tensors on otherwise valid arguments, where the VideoUpscaler's record is that of its first push."""
import torch

from savsr_amd import yuv
from savsr_amd.video import SAMPLE_FORMATS, layout_of

N, SIZE = 9, (12, 16)
NCH = (3, 1)
AXES = (
    ("pixel_format", ("rgb", "i420", "i422", "i444", "y400", "nv12")),
    ("out", ("float", "uint8", "i420", "i422", "i444", "y400", "rgb48")),
    ("size", (None, SIZE)),
    ("colour", ("bt601", "bt709-full", "bt2020")),
    ("out_colour", (None, "bt709", "bt601")),
    ("depth", (8, 10, 9)),
    ("out_depth", (None, 12)),
    ("siting", (None, "left", "topleft", "mpeg2")),
    ("out_siting", (None, "left", "topleft")),
    ("chroma_filter", (None, "bicubic", "lanczos")),
    ("cuts", (None, [4], [0])),
    ("scale", (None, -1.0)),
)
_SIZES = [len(NCH)] + [len(v) for _, v in AXES]
GRID_CASES = 1
for _s in _SIZES:
    GRID_CASES *= _s

_I420 = dict(pixel_format="i420", size=SIZE)
_FB = yuv.frame_bytes(SIZE[0], SIZE[1])
# (num_in_ch, arguments, frames): the tensor is wrong for the arguments in one way each
TENSOR_CASES = (
    (3, {}, lambda: [[0]]),                                                             # not a tensor
    (3, {}, lambda: torch.zeros(N, 12, 16, 3, dtype=torch.int32)),                      # dtype
    (3, {}, lambda: torch.zeros(N, 12, 16, dtype=torch.uint8)),                         # rank
    (3, {}, lambda: torch.zeros(N, 3, 12, 16)),                                         # float frames on the host
    (3, {}, lambda: torch.zeros(N, 12, 16, 1, dtype=torch.uint8)),                      # channels
    (3, {}, lambda: torch.zeros(N, 1, 16, 3, dtype=torch.uint8)),                       # h < 2
    (3, {}, lambda: torch.zeros(0, 12, 16, 3, dtype=torch.uint8)),                      # no frames
    (3, {}, lambda: torch.zeros(2, 12, 16, 3, dtype=torch.uint8)),                      # too few for the window
    (3, dict(cuts=[4]), lambda: torch.zeros(4, 12, 16, 3, dtype=torch.uint8)),          # a cut behind the end
    (3, _I420, lambda: None),
    (3, _I420, lambda: torch.zeros(N, _FB)),                                            # dtype
    (3, _I420, lambda: torch.zeros(N, 12, 16, 3, dtype=torch.uint8)),                   # rank
    (3, _I420, lambda: torch.zeros(N, _FB + 1, dtype=torch.uint8)),                     # byte count
    (3, dict(_I420, depth=10), lambda: torch.zeros(N, _FB, dtype=torch.uint8)),         # 8-bit frames at 10 bits
    (3, dict(pixel_format="i444", size=SIZE, depth=12), lambda: torch.zeros(N, 3 * 12 * 16, dtype=torch.uint8)),
    (3, dict(_I420, cuts="auto"), lambda: torch.zeros(0, _FB, dtype=torch.uint8)),      # no frames, with cuts
    (1, _I420, lambda: torch.zeros(N, _FB, dtype=torch.uint8)),                         # colour frames, luma network, no filter
    (1, dict(_I420, chroma_filter="bicubic", out="i420"), lambda: torch.zeros(N, _FB - 2, dtype=torch.uint8)),
    (1, dict(pixel_format="y400", size=SIZE, out="y400"), lambda: torch.zeros(N, _FB, dtype=torch.uint8)),      # I420 bytes as Y400
    (1, dict(pixel_format="y400", size=SIZE, depth=10), lambda: torch.zeros(N, 2, 12 * 16, dtype=torch.uint8)),
    (1, {}, lambda: torch.zeros(N, 12, 16, 3, dtype=torch.uint8)),                      # channels
    # a stage in front (fields= / pulldown=): its own refusals speak before the layout's, and the device before the rect
    (3, dict(fields="tff"), lambda: torch.zeros(N, 3, 12, 16)),                         # float frames: the stage, not "on the GPU"
    (3, dict(pulldown="tff"), lambda: torch.zeros(N, 1, 16, 3, dtype=torch.uint8)),     # one row: the stage, not h < 2
    (3, dict(fields="bff"), lambda: torch.zeros(N, 12, 16, 1, dtype=torch.uint8)),      # channels: the stage takes them, the layout not
    (3, dict(fields="tff", crop=(0, 0, 40, 40)), lambda: torch.zeros(N, 12, 16, 3, dtype=torch.uint8)),      # a rect that does not fit
    (3, dict(crop=(0, 0, 40, 40)), lambda: torch.zeros(N, 12, 16, 3, dtype=torch.uint8)),                    # the same without a stage
)
CASES = GRID_CASES + len(TENSOR_CASES)
CONSTRUCTED = ["constructed", ""]

_nets, _frames = {}, {}


def net_of(nch: int):
    if nch not in _nets:
        from savsr_amd.archs.savsr_arch import SAVSR
        _nets[nch] = SAVSR(num_in_ch=nch, num_feat=32).eval()
    return _nets[nch]


def grid_case(k: int):
    """(num_in_ch, arguments) of grid case k."""
    pos = []
    for s in reversed(_SIZES):
        k, r = divmod(k, s)
        pos.append(r)
    pos.reverse()
    return NCH[pos[0]], {name: values[p] for (name, values), p in zip(AXES, pos[1:])}


def grid_frames(nch: int, kw: dict) -> torch.Tensor:
    """The frames tensor of a grid case, right for its arguments where they allow one: planar frames of the layout and depth when the
    pixel format has planes and a size came with it (a depth that is none: 8 bits), N x 12 x 16 x num_in_ch uint8 frames otherwise."""
    fmt, depth = kw["pixel_format"], kw["depth"] if kw["depth"] in yuv.DEPTHS else 8
    key = (fmt, depth) if fmt in SAMPLE_FORMATS and kw["size"] is not None else nch
    if key not in _frames:
        _frames[key] = (torch.zeros(N, 12, 16, nch, dtype=torch.uint8) if key == nch else
                        torch.zeros(N, yuv.frame_bytes(SIZE[0], SIZE[1], depth, layout_of(fmt)), dtype=torch.uint8))
    return _frames[key]


def _outcome(fn):
    try:
        fn()
    except Exception as e:  # noqa: BLE001  (the census records whatever is raised)
        return [type(e).__name__, str(e)]
    return CONSTRUCTED


def record(k: int):
    """[upscale_video's outcome, VideoUpscaler's outcome] of case k, each [type name, message]."""
    from savsr_amd import VideoUpscaler
    if k < GRID_CASES:
        nch, kw = grid_case(k)
        net, frames = net_of(nch), grid_frames(nch, kw)
        return [_outcome(lambda: net.upscale_video(frames, **kw)), _outcome(lambda: VideoUpscaler(net, **kw))]
    nch, kw, make = TENSOR_CASES[k - GRID_CASES]
    net, frames = net_of(nch), make()
    return [_outcome(lambda: net.upscale_video(frames, **kw)), _outcome(lambda: VideoUpscaler(net, **kw).push(frames))]

