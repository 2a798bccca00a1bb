"""Raw YUV 4:2:0 without a GPU: savsr_amd/yuv.py (the restatement the I420 kernels are tested against) pinned by the REFERENCE's
ycbcr2rgb / rgb2ycbcr (tests/golden/yuv_outputs.npz, tools/gen_golden_yuv.py), the Y4M reader / writer (savsr_amd/y4m.py) and the
refusals of the I420 arguments and of the CLI (all of them raise before the GPU is touched)."""
import io
import os
import threading
from fractions import Fraction

import numpy as np
import pytest
import torch

from savsr_amd import y4m, yuv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(2, 2), (3, 5), (8, 10), (9, 14), (17, 33)]
TIE_EPS = 1e-4          # float32 evaluation error on values <= 255: about 6 ulp = 9e-5


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "yuv_outputs.npz"))


def test_frame_layout():
    assert yuv.i420_bytes(2, 2) == 6 and yuv.i420_bytes(3, 5) == 15 + 2 * 6 and yuv.i420_bytes(180, 320) == 180 * 320 * 3 // 2
    fr = np.arange(yuv.i420_bytes(3, 5), dtype=np.uint8)[None]
    y, u, v = yuv.split_planes(fr, 3, 5)
    assert y.shape == (1, 3, 5) and u.shape == (1, 2, 3) and v.shape == (1, 2, 3)
    assert y[0, 2, 4] == 14 and u[0, 0, 0] == 15 and v[0, 0, 0] == 21 and v[0, 1, 2] == 26
    with pytest.raises(ValueError, match=r"I420 frames of 3 x 5 are \[N, 27\] uint8"):
        yuv.split_planes(fr[:, :-1], 3, 5)


@pytest.mark.parametrize("name,h,w", [("table", 256, 256)] + [(f"{h}x{w}", h, w) for h, w in SIZES])
def test_i420_to_rgb_vs_reference_golden(gold, name, h, w):
    """<= 2e-6, derived: each channel is at most three float32 terms of magnitude < 4 summed and clamped, i.e. <= 6 roundings of half an
    ulp at [2, 4) = 2.4e-7 each."""
    got = yuv.i420_to_rgb(gold[f"in/{name}/i420"], h, w)
    ref = gold[f"in/{name}/rgb"]
    assert got.dtype == np.float32 and got.shape == ref.shape
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(name, "max-abs", err)
    assert err <= 2e-6
    assert got.min() >= 0.0 and got.max() <= 1.0


def test_table_frame_covers_every_luma_value_against_the_chroma_grid(gold):
    y, u, v = yuv.split_planes(gold["in/table/i420"], 256, 256)
    uu = np.repeat(np.repeat(u, 2, 1), 2, 2)
    vv = np.repeat(np.repeat(v, 2, 1), 2, 2)
    triples = set(zip(y.reshape(-1).tolist(), uu.reshape(-1).tolist(), vv.reshape(-1).tolist()))
    assert len(triples) == 256 * 16 * 16


def test_rgb_to_i420_vs_reference_golden(gold):
    """Samples away from a tie equal round(golden) exactly; a sample whose float64 value lies within 1e-4 of some k + 0.5 may differ by
    one.  The near-tie set comes from the golden alone and holds at most 0.1 % of the samples."""
    near = total = 0
    for h, w in SIZES:
        x = gold[f"out/{h}x{w}/rgb"]
        got = yuv.rgb_to_i420(x)
        assert got.dtype == np.uint8 and got.shape == (x.shape[0], yuv.i420_bytes(h, w))
        planes = yuv.split_planes(got, h, w)
        for p, key in zip(planes, ("y", "cb", "cr")):
            ref = gold[f"out/{h}x{w}/{key}"]
            assert ref.dtype == np.float64 and ref.shape == p.shape
            tie = np.abs(ref - np.floor(ref) - 0.5) <= TIE_EPS
            want = np.rint(ref)
            diff = np.abs(p.astype(np.float64) - want)
            assert (diff[~tie] == 0).all(), (h, w, key, float(diff[~tie].max()))
            assert (diff[tie] <= 1).all(), (h, w, key)
            near += int(tie.sum())
            total += tie.size
    print("near a tie:", near, "of", total)
    assert near <= 1e-3 * total


def test_rgb_to_i420_ranges_and_clamp():
    x = np.array([-5.0, 0.0, 1.0, 7.0], np.float32)
    img = np.stack(np.meshgrid(x, x, x, indexing="ij"), 0).reshape(3, 8, 8)[None]
    y, u, v = yuv.split_planes(yuv.rgb_to_i420(img), 8, 8)
    assert y.min() == 16 and y.max() == 235
    assert min(u.min(), v.min()) >= 16 and max(u.max(), v.max()) <= 240
    assert np.array_equal(yuv.rgb_to_i420(img), yuv.rgb_to_i420(np.clip(img, 0, 1)))
    extremes = np.array([[0, 0, 1], [1, 1, 0], [1, 0, 0], [0, 1, 1]], np.float32).T.reshape(1, 3, 1, 4)       # blue, yellow, red, cyan
    yy, cb, cr = yuv.ycbcr_f32(np.repeat(np.repeat(extremes, 2, 2), 2, 3))
    assert np.rint(cb).max() == 240 and np.rint(cb).min() == 16 and np.rint(cr).max() == 240 and np.rint(cr).min() == 16


@pytest.mark.parametrize("h,w", SIZES + [(180, 320), (181, 319)])
def test_idempotence_on_block_constant_images(h, w):
    """x constant on every 2 x 2 block with values in [8/255, 247/255] (no clamp acts on the way back): y = rgb_to_i420(x) is a fixed
    point of rgb_to_i420(i420_to_rgb(.)) -- the two matrices are inverse to ~1e-6 relative, ~3e-4 of an 8-bit step."""
    rng = np.random.RandomState(h * 1000 + w)
    ch, cw = yuv.chroma_hw(h, w)
    blocks = rng.uniform(8 / 255, 247 / 255, size=(2, 3, ch, cw)).astype(np.float32)
    x = np.repeat(np.repeat(blocks, 2, 2), 2, 3)[:, :, :h, :w]
    y = yuv.rgb_to_i420(x)
    back = yuv.i420_to_rgb(y, h, w)
    assert back.min() > 0.0 and back.max() < 1.0                    # (no clamp acted)
    assert np.array_equal(yuv.rgb_to_i420(back), y)


# ------------------------------------------------------------------------------------------------------------------------------ Y4M
def _frames(n, h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=(n, yuv.i420_bytes(h, w)), dtype=np.uint8)


@pytest.mark.parametrize("h,w", [(4, 6), (5, 7), (2, 2), (9, 14)])
def test_y4m_write_then_read_is_the_identity(h, w):
    fr = _frames(5, h, w, seed=h)
    f = io.BytesIO()
    wr = y4m.Y4MWriter(f, w, h, fps=(30000, 1001), interlace="p", aspect=(4, 3))
    wr.write(fr[:2])
    wr.write(fr[2:])
    data = f.getvalue()
    assert data.startswith(f"YUV4MPEG2 W{w} H{h} F30000:1001 Ip A4:3 C420jpeg\n".encode())
    assert len(data) == len(wr.header) + 5 * (6 + yuv.i420_bytes(h, w))
    rd = y4m.Y4MReader(io.BytesIO(data))
    assert (rd.width, rd.height, rd.fps, rd.interlace, rd.aspect, rd.colorspace) == (w, h, (30000, 1001), "p", (4, 3), "420jpeg")
    got = np.concatenate(list(rd.chunks(2)), 0)
    assert np.array_equal(got, fr) and rd.frames_read == 5


def test_y4m_reader_on_a_pipe_in_chunks_that_do_not_divide_the_length():
    h, w, n = 7, 9, 11
    fr = _frames(n, h, w, seed=3)
    src = io.BytesIO()
    y4m.Y4MWriter(src, w, h).write(fr)
    data = src.getvalue()
    r, wfd = os.pipe()

    def feed():
        with os.fdopen(wfd, "wb", buffering=0) as out:
            for a in range(0, len(data), 50):                     # short writes: a frame arrives in pieces
                out.write(data[a:a + 50])
    t = threading.Thread(target=feed)
    t.start()
    try:
        with io.BufferedReader(os.fdopen(r, "rb", buffering=0)) as pipe:
            assert not pipe.seekable()
            rd = y4m.Y4MReader(pipe)
            parts = list(rd.chunks(4))
    finally:
        t.join()
    assert [p.shape[0] for p in parts] == [4, 4, 3]
    assert np.array_equal(np.concatenate(parts, 0), fr)


def test_y4m_reader_on_an_unbuffered_object_without_readline():
    class Raw:                                          # read() only, at most 5 bytes a call
        def __init__(self, data):
            self.b = io.BytesIO(data)

        def read(self, n):
            return self.b.read(min(n, 5))
    fr = _frames(3, 3, 5)
    src = io.BytesIO()
    y4m.Y4MWriter(src, 5, 3).write(fr)
    assert np.array_equal(np.concatenate(list(y4m.Y4MReader(Raw(src.getvalue())).chunks(2)), 0), fr)


def _stream(header: bytes, frames=b"") -> io.BytesIO:
    return io.BytesIO(header + frames)


def test_y4m_header_tags():
    body = b"FRAME Ip Xextra\n" + bytes(6)                          # FRAME lines may carry parameters
    rd = y4m.Y4MReader(_stream(b"YUV4MPEG2 W2 H2 F25:1 Ip A1:1 XYSCSS=420JPEG XCOLORRANGE=LIMITED\n", body))
    assert (rd.width, rd.height, rd.colorspace) == (2, 2, "420")       # no C tag = 420; X tags ignored
    assert sum(c.shape[0] for c in rd.chunks(3)) == 1
    for tag in ("C420", "C420jpeg", "C420mpeg2", "C420paldv"):
        assert y4m.Y4MReader(_stream(b"YUV4MPEG2 W2 H2 F25:1 " + tag.encode() + b"\n")).colorspace == tag[1:]
    rd = y4m.Y4MReader(_stream(b"YUV4MPEG2 H4 W6\n"))
    assert (rd.height, rd.width, rd.fps, rd.aspect, rd.interlace) == (4, 6, (25, 1), (0, 0), "p")
    assert list(rd.chunks(2)) == []


@pytest.mark.parametrize("tag", ["C422", "C444", "C420p10", "Cmono", "C444alpha", "C411"])
def test_y4m_refuses_other_colour_spaces_by_name(tag):
    with pytest.raises(ValueError, match=f"colour space tag '{tag}' is not supported: 8-bit 4:2:0 only"):
        y4m.Y4MReader(_stream(b"YUV4MPEG2 W4 H4 F25:1 " + tag.encode() + b"\n"))


@pytest.mark.parametrize("header,match", [
    (b"RIFF....AVI \n", "not a YUV4MPEG2 stream"),
    (b"", "not a YUV4MPEG2 stream"),
    (b"YUV4MPEG2 W4 F25:1\n", "names no W / H"),
    (b"YUV4MPEG2 W0 H4\n", "bad header tag 'W0'"),
    (b"YUV4MPEG2 W4 H4 F25\n", "bad header tag F'25'"),
    (b"YUV4MPEG2 W4 H4 Q7\n", "unknown header tag 'Q7'"),
])
def test_y4m_refuses_bad_headers(header, match):
    with pytest.raises(ValueError, match=match):
        y4m.Y4MReader(_stream(header))


def test_y4m_truncated_last_frame_is_an_error_naming_the_frame():
    fr = _frames(3, 4, 6)
    src = io.BytesIO()
    y4m.Y4MWriter(src, 6, 4).write(fr)
    data = src.getvalue()
    rd = y4m.Y4MReader(io.BytesIO(data[:-5]))
    with pytest.raises(ValueError, match="frame 2 is truncated: 31 of 36 bytes"):
        list(rd.chunks(2))
    rd = y4m.Y4MReader(io.BytesIO(data[:-36 - 3]))                    # inside the last FRAME line
    with pytest.raises(ValueError, match="frame 2: 'FRAME' line expected"):
        list(rd.chunks(8))
    rd = y4m.Y4MReader(io.BytesIO(data.replace(b"FRAME\n", b"FRAMX\n", 1)))
    with pytest.raises(ValueError, match="frame 0: 'FRAME' line expected"):
        list(rd.chunks(1))


def test_y4m_aspect_keeps_the_display_aspect_under_an_asymmetric_scale():
    from savsr_amd.packing import get_hw
    h, w, sc = 180, 320, (3.5, 2.0)
    H, W = get_hw(h, w, sc)
    assert (H, W) == (630, 640)
    want = Fraction(1 * w * H, 1 * W * h)
    assert y4m.scaled_aspect((1, 1), (h, w), (H, W)) == (want.numerator, want.denominator) == (7, 4)
    assert Fraction(W * want.numerator, H * want.denominator) == Fraction(w, h)           # the display aspect is the LR video's
    assert y4m.scaled_aspect((0, 0), (h, w), (H, W)) == (0, 0)                           # unknown stays unknown
    want = Fraction(10 * w * H, 11 * W * h)
    assert y4m.scaled_aspect((10, 11), (h, w), (H, W)) == (want.numerator, want.denominator)
    assert y4m.scaled_aspect((1, 1), (h, w), (4 * h, 4 * w)) == (1, 1)
    f = io.BytesIO()
    y4m.Y4MWriter(f, W, H, (25, 1), "p", y4m.scaled_aspect((1, 1), (h, w), (H, W)))
    assert f.getvalue() == b"YUV4MPEG2 W640 H630 F25:1 Ip A7:4 C420jpeg\n"


def test_y4m_writer_refuses_frames_of_another_size():
    wr = y4m.Y4MWriter(io.BytesIO(), 6, 4)
    with pytest.raises(ValueError, match=r"frames of 4 x 6 are \[m, 36\] uint8"):
        wr.write(np.zeros((1, 35), np.uint8))


# ------------------------------------------------------------------------------------------------- the public interface, on the host
def _net(**cfg):
    from savsr_amd.archs.savsr_arch import SAVSR
    return SAVSR(**cfg).eval()


def _i420(n, h=8, w=10):
    return torch.zeros(n, yuv.i420_bytes(h, w), dtype=torch.uint8)


@pytest.mark.parametrize("kwargs,frames,match", [
    (dict(pixel_format="nv12", size=(8, 10)), _i420(9), "pixel_format = 'nv12': one of rgb, i420"),
    (dict(pixel_format="i420"), _i420(9), "pixel_format = 'i420' needs size = \\(h, w\\), got None"),
    (dict(pixel_format="i420", size=8), _i420(9), "needs size = \\(h, w\\), got 8"),
    (dict(pixel_format="i420", size=(8.5, 10)), _i420(9), "needs size = \\(h, w\\)"),
    (dict(size=(8, 10)), torch.zeros(9, 8, 10, 3, dtype=torch.uint8), "size = \\(h, w\\) goes with pixel_format = 'i420'"),
    (dict(pixel_format="i420", size=(1, 10)), _i420(9, 1, 10), "SAVSR needs h, w >= 2, got 1 x 10"),
    (dict(pixel_format="i420", size=(8, 10)), _i420(9, 8, 12), "I420 frames of 8 x 10 have 120 bytes, got 144"),
    (dict(pixel_format="i420", size=(8, 10)), _i420(9).float(), "I420 frames must be uint8"),
    (dict(pixel_format="i420", size=(8, 10)), _i420(9)[0], "got 1 dimensions"),
    (dict(pixel_format="i420", size=(8, 10)), _i420(3), "video has 3 frames: too few for a 7-frame 'reflection' window"),
    (dict(pixel_format="i420", size=(8, 10), out="yuv"), _i420(9), "out = 'yuv': one of float, uint8, i420"),
])
def test_upscale_video_refuses_bad_i420_arguments_without_a_gpu(kwargs, frames, match):
    with pytest.raises(ValueError, match=match):
        _net().upscale_video(frames, **kwargs)


def test_i420_needs_a_colour_network():
    net = _net(num_in_ch=1)
    with pytest.raises(ValueError, match="I420 frames are colour frames, the network takes num_in_ch = 1"):
        net.upscale_video(_i420(9), pixel_format="i420", size=(8, 10))
    with pytest.raises(ValueError, match="out = 'i420' holds colour frames"):
        net.upscale_video(torch.zeros(9, 8, 10, 1, dtype=torch.uint8), out="i420")
    with pytest.raises(RuntimeError, match="AMD GPU only"):           # every host check passed: only the device is missing
        _net().upscale_video(_i420(9), pixel_format="i420", size=(8, 10), out="i420")


def test_video_upscaler_takes_the_same_two_arguments():
    from savsr_amd import VideoUpscaler
    with pytest.raises(ValueError, match="needs size"):
        VideoUpscaler(_net(), 4, pixel_format="i420")
    up = VideoUpscaler(_net(), 4, out="i420", pixel_format="i420", size=(8, 10))
    assert up.i420 == (8, 10) and up.out == "i420"
    with pytest.raises(ValueError, match="have 120 bytes, got 119"):
        up.push(_i420(2)[:, :-1])
    with pytest.raises(ValueError, match="the video has no frames"):
        up.finish()
    assert VideoUpscaler(_net(), 4).i420 is None


def test_cli_y4m_arguments():
    from savsr_amd.upscale import is_y4m, parse_args
    assert is_y4m("-") and is_y4m("a/b.y4m") and is_y4m("X.Y4M") and not is_y4m("frames/") and not is_y4m("y4m")
    base = ["--scale", "4", "--checkpoint", "x.pth"]
    a = parse_args(["-i", "-", "-o", "-"] + base)
    assert a.y4m_in and a.y4m_out and a.fps == (25, 1)
    a = parse_args(["-i", "lr", "-o", "out.y4m", "--fps", "30000:1001"] + base)
    assert not a.y4m_in and a.y4m_out and a.fps == (30000, 1001)
    assert parse_args(["-i", "lr", "-o", "out.y4m", "--fps", "24"] + base).fps == (24, 1)
    a = parse_args(["-i", "in.y4m", "-o", "sr"] + base)
    assert a.y4m_in and not a.y4m_out
    for bad in (["-i", "in.y4m", "-o", "out.y4m", "--fps", "25"],            # a Y4M input carries its frame rate
                ["-i", "lr", "-o", "sr", "--fps", "25"],                      # PNGs have none
                ["-i", "lr", "-o", "out.y4m", "--fps", "0"],
                ["-i", "lr", "-o", "out.y4m", "--fps", "25:0"],
                ["-i", "lr", "-o", "out.y4m", "--fps", "ntsc"]):
        with pytest.raises(SystemExit):
            parse_args(bad + base)
