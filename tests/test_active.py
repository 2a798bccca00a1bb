"""The active picture of letterboxed video, host side (savsr_amd/active.py, no GPU): the line sums against plain loops, cropdetect's
rule on both sides of its threshold, the alignment and the placement rules, the crop / insert round trip, every refusal of the new
arguments on a CPU network, the command line's parsing and the Y4M header of --bars drop."""
import io
import random
from fractions import Fraction

import numpy as np
import pytest
import torch

import savsr_amd
from savsr_amd import active, upscale, y4m, yuv
from savsr_amd.packing import get_hw
from savsr_amd.utils import workloads
from savsr_amd.video import layout_of

LAYOUTS = ("420", "422", "444", yuv.MONO)
FMT = {"420": "i420", "422": "i422", "444": "i444", yuv.MONO: "y400"}


# ---------------------------------------------------------------------------------------------------------------------- line_sums
def _loops(samples):
    """samples[n][y][x] = list of the 8-bit samples at that position -> (rows, cols) by plain loops."""
    n, h, w = len(samples), len(samples[0]), len(samples[0][0])
    rows = [[sum(sum(samples[f][y][x]) for x in range(w)) for y in range(h)] for f in range(n)]
    cols = [[sum(sum(samples[f][y][x]) for y in range(h)) for x in range(w)] for f in range(n)]
    return np.array(rows, np.int64), np.array(cols, np.int64)


def test_line_sums_of_packed_uint8_frames():
    v = np.random.RandomState(0).randint(0, 256, size=(3, 5, 3, 3), dtype=np.uint8)
    rows, cols = active.line_sums(v)
    want = _loops([[[[int(b) for b in v[f, y, x]] for x in range(3)] for y in range(5)] for f in range(3)])
    assert rows.dtype == cols.dtype == np.int64 and rows.shape == (3, 5) and cols.shape == (3, 3)
    assert np.array_equal(rows, want[0]) and np.array_equal(cols, want[1])
    assert np.array_equal(active.line_sums(torch.from_numpy(v))[0], rows)


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_line_sums_of_planar_frames_read_the_luma_plane(layout, depth):
    h, w, n = 5, 7, 3
    rng = np.random.RandomState(depth + int(layout))
    ns = yuv.frame_bytes(h, w, 8, layout)          # samples per frame
    s = rng.randint(0, 1 << depth, size=(n, ns)).astype(np.uint16)
    if depth != 8:
        s[:, ::5] = rng.randint(1 << depth, 1 << 16, size=s[:, ::5].shape)          # above 2^d - 1: read as 2^d - 1
        frames = s.astype("<u2").view(np.uint8).reshape(n, -1)
    else:
        frames = s.astype(np.uint8)
    rows, cols = active.line_sums(frames, FMT[layout], (h, w), depth)
    want = _loops([[[[min(int(s[f, y * w + x]), (1 << depth) - 1) >> (depth - 8)] for x in range(w)] for y in range(h)] for f in range(n)])
    assert np.array_equal(rows, want[0]) and np.array_equal(cols, want[1])


def test_line_sums_of_float_frames_quantise_first():
    v = np.random.RandomState(1).uniform(-0.5, 1.5, size=(2, 3, 4, 5)).astype(np.float32)
    v[0, 0, 0, 0], v[1, 2, 3, 4], v[0, 1, 2, 3], v[1, 0, 1, 1] = np.nan, -0.5, 1.5, 0.5 / 255          # NaN -> 0, < 0 -> 0, > 1 -> 255, tie -> even
    assert (v < 0).any() and (v > 1).any() and np.isnan(v).any()

    def q(x):
        x = np.float32(x)
        if np.isnan(x):
            return 0
        return int(np.rint(np.float32(min(max(x, np.float32(0)), np.float32(1))) * np.float32(255)))
    rows, cols = active.line_sums(v)
    want = _loops([[[[q(v[f, c, y, x]) for c in range(3)] for x in range(5)] for y in range(4)] for f in range(2)])
    assert np.array_equal(rows, want[0]) and np.array_equal(cols, want[1])
    assert want[0][0][0] == sum(q(v[0, c, 0, x]) for c in range(3) for x in range(5))


# ---------------------------------------------------------------------------------------------------------------------- active_rect
def test_active_rect_on_both_sides_of_the_threshold():
    limit, s_row, s_col = 24.5, 6, 8          # limit * S: 147 per row, 196 per column
    assert Fraction(limit) * s_row == 147 and Fraction(limit) * s_col == 196
    rows, cols = [0] * 8, [0] * 6
    rows[2], rows[5], cols[1], cols[4] = 148, 148, 197, 197
    assert active.active_rect(rows, cols, s_row, s_col, limit) == (2, 1, 4, 4)
    rows[1], cols[5] = 147, 196                # exactly the limit: black
    assert active.active_rect(rows, cols, s_row, s_col, limit) == (2, 1, 4, 4)
    rows[1], cols[5] = 148, 197                # one more: picture
    assert active.active_rect(rows, cols, s_row, s_col, limit) == (1, 1, 5, 5)
    assert active.active_rect(rows, cols, s_row, s_col, Fraction(49, 2)) == (1, 1, 5, 5)
    assert active.active_rect(rows, cols, s_row, s_col) == (1, 1, 5, 5)          # the default: 24
    assert active.DEFAULT_LIMIT == 24


def test_a_bar_line_bright_in_one_frame_of_nine_is_picture():
    v = np.full((9, 12, 10, 1), 16, np.uint8)
    v[:, 3:9, 2:8] = 100
    rows, cols = active.line_sums(v)
    assert active.active_rect(rows.max(0), cols.max(0), 10, 12) == (3, 2, 6, 6)
    v[4, 1, :] = 200                           # a bright line inside the top bar, in one frame only
    rows, cols = active.line_sums(v)
    assert active.active_rect(rows.max(0), cols.max(0), 10, 12) == (1, 0, 8, 10)


def test_all_black_and_one_row_pictures_give_the_whole_frame():
    v = np.full((9, 12, 10, 3), 16, np.uint8)
    rows, cols = active.line_sums(v)
    assert active.active_rect(rows.max(0), cols.max(0), 30, 36) == (0, 0, 12, 10)
    v[:, 5, 2:8] = 255                         # a 1-row picture: below 2 x 2
    rows, cols = active.line_sums(v)
    assert active.active_rect(rows.max(0), cols.max(0), 30, 36) == (0, 0, 12, 10)
    v[:, 6, 2:8] = 255                         # two rows: a picture
    rows, cols = active.line_sums(v)
    assert active.active_rect(rows.max(0), cols.max(0), 30, 36) == (5, 2, 2, 6)


def test_limit_is_checked():
    for bad in (None, "24", True, float("nan"), float("inf"), -1, 255, 300.0):
        with pytest.raises(ValueError, match="crop_limit"):
            active.check_limit(bad)
    assert active.check_limit(0) == 0 and active.check_limit(24.5) == Fraction(49, 2)


# ---------------------------------------------------------------------------------------------------------------------- align_rect
def test_align_rect_moves_odd_offsets_outwards():
    rect = (3, 5, 10, 11)
    assert active.align_rect(rect, "420") == (2, 4, 11, 12)
    assert active.align_rect(rect, "422") == (3, 4, 10, 12)
    for layout in ("444", yuv.MONO, None):
        assert active.align_rect(rect, layout) == rect
    assert active.align_rect((2, 4, 11, 13), "420") == (2, 4, 11, 13)          # odd sizes stay: the far edge does not move
    for layout in LAYOUTS + (None,):
        y0, x0, ah, aw = active.align_rect(rect, layout)
        assert y0 <= 3 and x0 <= 5 and y0 + ah == 13 and x0 + aw == 16             # never inwards
    with pytest.raises(ValueError):
        active.align_rect(rect, "411")


# ---------------------------------------------------------------------------------------------------------------------- place
def _check_place(h, w, rect, scale, layout):
    Hf, Wf, Ha, Wa, Y0, X0 = active.place(rect, h, w, scale, layout)
    bv, bh = active.block_of(layout)
    assert (Hf, Wf) == get_hw(h, w, scale) and (Ha, Wa) == get_hw(rect[2], rect[3], scale)
    assert 0 <= Y0 and Y0 % bv == 0 and Y0 + Ha <= Hf, (h, w, rect, scale, layout)
    assert 0 <= X0 and X0 % bh == 0 and X0 + Wa <= Wf, (h, w, rect, scale, layout)


def test_place_over_the_yaml_and_training_scale_lists():
    assert len(workloads.YAML_SCALES) == 42 and len(workloads.TRAIN_SCALES) == 60
    for scale in workloads.YAML_SCALES + workloads.TRAIN_SCALES:
        for layout in LAYOUTS + (None,):
            _check_place(180, 320, (22, 0, 136, 320), scale, layout)          # the letterbox of the measurements
            _check_place(180, 320, (0, 40, 180, 240), scale, layout)          # a pillarbox
            _check_place(181, 319, (20, 38, 161, 281), scale, layout)         # odd everything, the far edges at the frame's
    assert active.place((22, 0, 136, 320), 180, 320, (4.0, 4.0), "420") == (720, 1280, 544, 1280, 88, 0)
    assert active.place((3, 5, 7, 9), 16, 20, (2.5, 3.0), "444") == (40, 60, 18, 27, 8, 15)          # round(7.5) = 8: half to even
    assert active.place((3, 5, 7, 9), 16, 20, (2.5, 3.0), "420") == (40, 60, 18, 27, 8, 16)          # 2 * round(3.75), 2 * round(7.5)


def test_place_on_random_rects():
    rng = random.Random(42)
    for _ in range(10000):
        h, w = rng.randint(2, 400), rng.randint(2, 400)
        ah, aw = rng.randint(2, h), rng.randint(2, w)
        rect = (rng.randint(0, h - ah), rng.randint(0, w - aw), ah, aw)
        scale = (rng.choice([1.0, 1.5, 2.0, 2.5, 3.3, 4.0, 7.9, rng.uniform(1, 8)]), rng.choice([1.0, 1.1, 2.5, 3.0, 4.0, rng.uniform(1, 8)]))
        _check_place(h, w, rect, scale, rng.choice(LAYOUTS + (None,)))


# ---------------------------------------------------------------------------------------------------------------------- crop / insert
@pytest.mark.parametrize("case", [("float", 8), ("uint8", 8), ("i420", 8), ("i420", 10), ("i422", 12), ("i444", 8), ("y400", 10)])
@pytest.mark.parametrize("ha", [11, 12])
def test_insert_then_crop_is_the_identity(case, ha):
    out, depth = case
    rng = np.random.RandomState(ha)
    layout = layout_of(out) if out in ("i420", "i422", "i444", "y400") else None
    placed = (40, 60, ha, 13, 8, 16)          # an odd H_a in 4:2:0 among them; Y0, X0 on every layout's block
    if out == "float":
        x = rng.rand(2, 3, ha, 13).astype(np.float32) + 0.5
    elif out == "uint8":
        x = rng.randint(1, 256, size=(2, ha, 13, 3), dtype=np.uint8)
    else:
        x = rng.randint(1, 256, size=(2, yuv.frame_bytes(ha, 13, depth, layout)), dtype=np.uint8)
    full = active.insert_frames(x, placed, out, depth)
    rect = (8, 16, ha, 13)
    if layout is None:
        assert full.shape == ((2, 3, 40, 60) if out == "float" else (2, 40, 60, 3))
        back = active.crop_frames(full, rect, out)
        assert np.count_nonzero(full) == x.size                                   # the bars are 0
    else:
        assert full.shape == (2, yuv.frame_bytes(40, 60, depth, layout))
        back = active.crop_frames(full, rect, out, (40, 60), depth)
        k = 1 << (depth - 8)
        planes = active._planes(full, 40, 60, depth, layout)
        assert planes[0][0, 0, 0] == 16 * k and planes[0][1, 39, 59] == 16 * k      # nominal black, limited range
        if layout != yuv.MONO:
            assert planes[1][0, 0, 0] == 128 * k and planes[2][1, -1, -1] == 128 * k
    assert back.dtype == x.dtype and np.array_equal(back, x)


def test_an_odd_picture_height_in_420_covers_the_first_bar_row_with_its_last_chroma_row():
    x = np.full((1, yuv.frame_bytes(11, 13)), 200, np.uint8)
    full = active.insert_frames(x, (40, 60, 11, 13, 8, 16), "i420")
    y, u, v = yuv.split_planes(full, 40, 60)
    assert (y[0, 8:19, 16:29] == 200).all() and y[0, 19, 16] == 16                 # luma row 19 is bar ...
    assert (u[0, 4:10, 8:15] == 200).all() and u[0, 10, 8] == 128                  # ... under chroma row 9 (luma rows 18, 19) of the picture
    assert (v[0, 4:10, 8:15] == 200).all()
    full = active.insert_frames(x, (40, 60, 11, 13, 8, 16), "i420", colour="bt709-full")
    assert yuv.split_planes(full, 40, 60)[0][0, 0, 0] == 0                         # full range: Y = 0


def test_crop_frames_of_planar_frames_crops_every_plane_at_its_block():
    h, w = 8, 10
    yp = np.arange(h * w, dtype=np.uint8).reshape(1, h, w)
    up = 100 + np.arange(20, dtype=np.uint8).reshape(1, 4, 5)
    vp = 150 + np.arange(20, dtype=np.uint8).reshape(1, 4, 5)
    frames = np.concatenate([p.reshape(1, -1) for p in (yp, up, vp)], 1)
    got = active.crop_frames(frames, (2, 4, 5, 5), "i420", (h, w))
    y, u, v = yuv.split_planes(got, 5, 5)
    assert np.array_equal(y, yp[:, 2:7, 4:9]) and np.array_equal(u, up[:, 1:4, 2:5]) and np.array_equal(v, vp[:, 1:4, 2:5])
    with pytest.raises(ValueError, match="aligned rect is \\(2, 4, 6, 5\\)"):
        active.crop_frames(frames, (3, 4, 5, 5), "i420", (h, w))


# ---------------------------------------------------------------------------------------------------------------------- refusals
@pytest.fixture(scope="module")
def net():
    from savsr_amd.archs.savsr_arch import SAVSR
    return SAVSR(num_feat=32).eval()


FRAMES = torch.zeros(9, 12, 16, 3, dtype=torch.uint8)
I420 = dict(pixel_format="i420", size=(12, 16), out="i420")
I420_FRAMES = torch.zeros(9, yuv.frame_bytes(12, 16), dtype=torch.uint8)


@pytest.mark.parametrize("kw,frames,words", [
    (dict(crop=(2, 2, 8, 20)), FRAMES, "does not lie inside the 12 x 16 frame"),
    (dict(crop=(8, 2, 8, 4)), FRAMES, "does not lie inside the 12 x 16 frame"),
    (dict(crop=(2, 2, 1, 8)), FRAMES, "ah, aw >= 2"),
    (dict(crop=(-2, 2, 4, 8)), FRAMES, "y0, x0 >= 0"),
    (dict(crop=(2, 2, 8)), FRAMES, "a rect \\(y0, x0, ah, aw\\) of ints"),
    (dict(crop=(2.0, 2, 8, 8)), FRAMES, "a rect \\(y0, x0, ah, aw\\) of ints"),
    (dict(crop="detect"), FRAMES, "None, 'auto' or a rect"),
    (dict(crop=(1, 2, 8, 8), **I420), I420_FRAMES, "off the chroma block of 4:2:0 frames .* the aligned rect is \\(0, 2, 9, 8\\)"),
    (dict(crop=(2, 3, 8, 8), **I420), I420_FRAMES, "the aligned rect is \\(2, 2, 8, 9\\)"),
    (dict(crop=(2, 3, 8, 8), pixel_format="i422", size=(12, 16)), torch.zeros(9, yuv.frame_bytes(12, 16, 8, "422"), dtype=torch.uint8),
     "off the chroma block of 4:2:2 frames"),
    (dict(bars="drop"), FRAMES, "bars = 'drop' goes with crop="),
    (dict(crop_limit=30), FRAMES, "crop_limit = 30 goes with crop="),
    (dict(crop="auto", bars="pad"), FRAMES, "bars = 'pad': one of keep, drop"),
    (dict(crop="auto", crop_limit=-3), FRAMES, "crop_limit must be in 0 <= limit < 255"),
    (dict(crop="auto", crop_limit="24"), FRAMES, "crop_limit must be a number"),
])
def test_upscale_video_refuses_by_name(net, kw, frames, words):
    with pytest.raises(ValueError, match=words):
        net.upscale_video(frames, **kw)


@pytest.mark.parametrize("kw,frames", [
    (dict(crop=(2, 3, 7, 9)), FRAMES),
    (dict(crop=(1, 3, 8, 8), pixel_format="i444", size=(12, 16)), torch.zeros(9, 3 * 12 * 16, dtype=torch.uint8)),
    (dict(crop=(2, 4, 7, 9), bars="drop", **I420), I420_FRAMES),
    (dict(crop="auto", crop_limit=30.5, bars="drop", cuts="auto"), FRAMES),
    (dict(crop=(0, 0, 12, 16)), FRAMES),
    (dict(crop=None, crop_limit=24, bars="keep"), FRAMES),
])
def test_a_valid_call_ends_at_the_gpu_only_error(net, kw, frames):
    with pytest.raises(RuntimeError, match="runs on an AMD GPU only"):
        net.upscale_video(frames, **kw)


def test_video_upscaler_takes_an_explicit_rect_only(net):
    from savsr_amd import VideoUpscaler
    with pytest.raises(ValueError, match="crop = 'auto' in VideoUpscaler: the decision needs the whole video.*detect_active_area"):
        VideoUpscaler(net, crop="auto")
    with pytest.raises(ValueError, match="bars = 'drop' goes with crop="):
        VideoUpscaler(net, bars="drop")
    with pytest.raises(ValueError, match="the aligned rect is \\(0, 2, 9, 8\\)"):
        VideoUpscaler(net, crop=(1, 2, 8, 8), **I420)          # planar chunks: the size is known at once
    with pytest.raises(ValueError, match="does not lie inside the 12 x 16 frame"):
        VideoUpscaler(net, crop=(2, 2, 8, 20), **I420)
    up = VideoUpscaler(net, crop=(2, 2, 8, 20))                # packed chunks carry the size: refused at the first push
    with pytest.raises(ValueError, match="does not lie inside the 12 x 16 frame"):
        up.push(FRAMES)
    up = VideoUpscaler(net, crop=(2, 4, 7, 9), bars="drop", **I420)
    assert up.spec.size == (7, 9) and up.spec.inp.layout == "420"          # the engine's spec is the cropped size's
    with pytest.raises(ValueError, match="I420 frames of 12 x 16 have 288 bytes, got 103"):
        up.push(torch.zeros(3, yuv.frame_bytes(7, 9), dtype=torch.uint8))          # chunks are checked against the full frame
    with pytest.raises(RuntimeError, match="runs on an AMD GPU only"):
        up.push(I420_FRAMES)
    assert VideoUpscaler(net, crop=(0, 0, 12, 16), **I420).spec.size == (12, 16)    # the whole frame: the uncropped path


def test_detector_entry_points_check_before_the_gpu():
    assert {"line_sums", "detect_active_area"} <= set(dir(savsr_amd))
    with pytest.raises(ValueError, match="crop_limit"):
        savsr_amd.detect_active_area(FRAMES, limit=-1)
    with pytest.raises(ValueError, match="frames must be uint8 or float"):
        savsr_amd.line_sums(torch.zeros(2, 4, 4, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="I420 frames of 12 x 16 are \\[N, 288\\] uint8"):
        savsr_amd.line_sums(torch.zeros(2, 100, dtype=torch.uint8), "i420", (12, 16))
    with pytest.raises(ValueError, match="float frames must be on the GPU"):
        savsr_amd.detect_active_area(torch.zeros(2, 3, 4, 4))


# ---------------------------------------------------------------------------------------------------------------------- the CLI
BASE = ["-i", "in.y4m", "-o", "out.y4m", "--scale", "2", "--checkpoint", "x.pth"]


def test_cli_parses_the_crop_options():
    a = upscale.parse_args(BASE)
    assert a.crop is None and a.bars == "keep" and a.crop_limit == 24
    a = upscale.parse_args(BASE + ["--crop", "auto"])
    assert a.crop == "auto" and a.bars == "keep" and a.crop_limit == 24
    a = upscale.parse_args(BASE + ["--crop", "auto", "--crop-limit", "30.5", "--bars", "drop"])
    assert a.crop == "auto" and a.bars == "drop" and a.crop_limit == 30.5
    a = upscale.parse_args(BASE + ["--crop", "22,0,136,320", "--bars", "drop"])
    assert a.crop == (22, 0, 136, 320) and a.bars == "drop"
    a = upscale.parse_args(["-i", "-", "-o", "-", "--scale", "2", "--checkpoint", "x.pth", "--crop", "2, 4, 11, 13"])
    assert a.crop == (2, 4, 11, 13)                         # an explicit rect works on a pipe


@pytest.mark.parametrize("extra,words", [
    (["--crop", "1,2,3"], "auto or Y0,X0,H,W"),
    (["--crop", "a,b,c,d"], "with integers"),
    (["--crop", "0,0,1,8"], "ah, aw >= 2"),
    (["--crop", "auto", "--crop-limit", "300"], "crop_limit must be in 0 <= limit < 255"),
    (["--crop", "2,4,11,13", "--crop-limit", "30"], "--crop-limit goes with --crop auto"),
    (["--bars", "drop"], "--crop-limit and --bars go with --crop"),
    (["--crop-limit", "30"], "--crop-limit and --bars go with --crop"),
    (["--crop", "auto", "--bars", "pad"], "invalid choice"),
])
def test_cli_refuses(extra, words, capsys):
    with pytest.raises(SystemExit):
        upscale.parse_args(BASE + extra)
    assert words in capsys.readouterr().err


def test_cli_refuses_crop_auto_on_stdin(capsys):
    with pytest.raises(SystemExit):
        upscale.parse_args(["-i", "-", "-o", "out.y4m", "--scale", "2", "--checkpoint", "x.pth", "--crop", "auto"])
    err = capsys.readouterr().err
    assert "--crop auto needs a first pass over the input, which stdin does not allow" in err and "--crop Y0,X0,H,W" in err


def test_y4m_header_with_bars_drop_carries_the_picture_size():
    h, w, rect, scale = 180, 320, (22, 0, 136, 320), (4.0, 4.0)
    assert upscale.written_lr(h, w, None, "keep") == (h, w) == upscale.written_lr(h, w, rect, "keep")
    lr = upscale.written_lr(h, w, rect, "drop")
    assert lr == (136, 320)
    H, W = get_hw(lr[0], lr[1], scale)
    f = io.BytesIO()
    y4m.Y4MWriter(f, W, H, (25, 1), "p", y4m.scaled_aspect((1, 1), lr, (H, W)))
    assert f.getvalue() == b"YUV4MPEG2 W1280 H544 F25:1 Ip A1:1 C420jpeg\n"
    lr, scale = upscale.written_lr(24, 32, (4, 0, 16, 32), "drop"), (2.5, 3.0)          # an asymmetric scale changes the pixel aspect
    H, W = get_hw(lr[0], lr[1], scale)
    f = io.BytesIO()
    y4m.Y4MWriter(f, W, H, (30, 1), "p", y4m.scaled_aspect((1, 1), lr, (H, W)))
    assert f.getvalue() == b"YUV4MPEG2 W96 H40 F30:1 Ip " + "A{}:{}".format(*y4m.scaled_aspect((1, 1), (16, 32), (40, 96))).encode() + b" C420jpeg\n"
    assert y4m.scaled_aspect((1, 1), (16, 32), (40, 96)) != (1, 1)
