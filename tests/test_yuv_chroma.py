"""YUV 4:2:2 and 4:4:4 without a GPU: the chroma= half of savsr_amd/yuv.py (the restatement savsr_video_gather_yuvp /
savsr_video_quantize_yuvp are tested against) pinned by the reference's ycbcr2rgb / rgb2ycbcr (tests/golden/yuv_chroma_outputs.npz,
tools/gen_golden_yuv_chroma.py) and, bit for bit, by the 4:2:0 code that tests/test_yuv.py pins; the Y4M reader / writer at C422 / C444
and their p10 / p12 forms; the refusals of the new arguments (all of them raise before the GPU is touched)."""
import io
import os
import threading

import numpy as np
import pytest
import torch

from savsr_amd import scenes, y4m, yuv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(2, 2), (3, 5), (8, 10), (9, 14), (17, 33)]
LAYOUTS = ("422", "444")
ALL = ("420", "422", "444")
DEPTHS = (8, 10, 12)
TIE_EPS = 1e-4          # float32 evaluation error on values <= 255: about 6 ulp = 9e-5 (tests/test_yuv.py)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "yuv_chroma_outputs.npz"))


def _colours(depth):
    return yuv.COLOURS if depth == 8 else ("bt601", "bt709")


def _frames(n, h, w, depth, chroma, seed=0):
    """n frames of random in-range samples of the layout and depth, [n, frame_bytes] uint8."""
    ns = yuv.frame_bytes(h, w, 8, chroma)
    s = np.random.RandomState(seed).randint(0, 1 << depth, size=(n, ns))
    return s.astype(np.uint8) if depth == 8 else s.astype("<u2").view(np.uint8)


def _join(planes, depth):
    n = planes[0].shape[0]
    flat = np.concatenate([np.asarray(p).reshape(n, -1) for p in planes], 1)
    return flat.astype(np.uint8) if depth == 8 else flat.astype("<u2").view(np.uint8)


def replicated(fr420, h, w, depth, chroma):
    """The 4:2:2 / 4:4:4 frames that hold a 4:2:0 frame's chroma by nearest replication (rows for 4:2:2, rows and columns for 4:4:4)."""
    y, u, v = yuv.split_planes(fr420, h, w, depth)
    if chroma == "422":
        u, v = (np.repeat(p, 2, axis=1)[:, :h] for p in (u, v))
    else:
        u, v = (yuv.replicate_chroma(p, h, w) for p in (u, v))
    return _join((y, u, v), depth)


# ----------------------------------------------------------------------------------------------------------------- layout and refusals
@pytest.mark.parametrize("h,w", [(2, 2), (3, 5), (180, 320)])
def test_frame_layout_of_every_layout_and_depth(h, w):
    want = {"420": ((h + 1) // 2, (w + 1) // 2), "422": (h, (w + 1) // 2), "444": (h, w)}
    for chroma in ALL:
        ch, cw = yuv.chroma_hw(h, w, chroma)
        assert (ch, cw) == want[chroma]
        for depth in DEPTHS:
            fb = yuv.frame_bytes(h, w, depth, chroma)
            assert fb == (h * w + 2 * ch * cw) * (1 if depth == 8 else 2)
            fr = _frames(2, h, w, depth, chroma, seed=h)
            assert fr.shape == (2, fb)
            y, u, v = yuv.split_planes(fr, h, w, depth, chroma)
            assert y.shape == (2, h, w) and u.shape == v.shape == (2, ch, cw)
            assert y.dtype == u.dtype == (np.uint8 if depth == 8 else np.uint16)
            s = fr if depth == 8 else fr.view("<u2")
            assert y[1, h - 1, w - 1] == s[1, h * w - 1] and u[1, 0, 0] == s[1, h * w] and v[1, ch - 1, cw - 1] == s[1, -1]
            name = ("" if depth == 8 else f"{depth}-bit ") + "I" + chroma
            with pytest.raises(ValueError, match=rf"{name} frames of {h} x {w} are \[N, {fb}\] uint8"):
                yuv.split_planes(fr[:, :-2], h, w, depth, chroma)
    assert yuv.frame_bytes(h, w) == yuv.i420_bytes(h, w) and yuv.frame_bytes(h, w, 10) == yuv.i420_bytes(h, w, 10)
    assert yuv.chroma_hw(h, w) == want["420"]


def test_chroma_names_are_checked():
    assert [yuv.check_chroma(c) for c in ALL] == [0, 1, 2] and yuv.CHROMAS == ALL
    for bad in ("411", 422, None, "i422"):
        with pytest.raises(ValueError, match="chroma = .*: one of 420, 422, 444"):
            yuv.check_chroma(bad)
    with pytest.raises(ValueError, match="chroma = '440': one of 420, 422, 444"):
        yuv.rgb_to_i420(np.zeros((1, 3, 2, 2), np.float32), chroma="440")
    with pytest.raises(ValueError, match="one of 420, 422, 444"):
        yuv.i420_to_rgb(np.zeros((1, 12), np.uint8), 2, 2, chroma="440")
    with pytest.raises(ValueError, match="depth = 10 with colour = 'bt709-full': 10 and 12 bits are defined for limited range only"):
        yuv.rgb_to_i420(np.zeros((1, 3, 2, 2), np.float32), "bt709-full", 10, "444")


# ---------------------------------------------------------------------------------------------------------------- against the golden
@pytest.mark.parametrize("chroma", LAYOUTS)
@pytest.mark.parametrize("h,w", SIZES)
def test_to_rgb_vs_reference_golden(gold, chroma, h, w):
    """<= 2e-6: the bound tests/test_yuv.py derives for the same arithmetic (<= 6 roundings of half an ulp at [2, 4) = 2.4e-7 each)."""
    got = yuv.i420_to_rgb(gold[f"in/{chroma}/{h}x{w}/yuv"], h, w, chroma=chroma)
    ref = gold[f"in/{chroma}/{h}x{w}/rgb"]
    assert got.dtype == np.float32 and got.shape == ref.shape == (3, 3, h, w)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(chroma, (h, w), "max-abs", err)
    assert err <= 2e-6
    assert got.min() >= 0.0 and got.max() <= 1.0


def test_from_rgb_vs_reference_golden(gold):
    """Samples away from a tie equal rint(golden) exactly; a sample whose float64 value lies within 1e-4 of some k + 0.5 may differ by
    one.  The near-tie set comes from the golden alone and holds at most 0.1 % of the samples."""
    near = total = 0
    for chroma in LAYOUTS:
        for h, w in SIZES:
            x = gold[f"out/{h}x{w}/rgb"]
            got = yuv.rgb_to_i420(x, chroma=chroma)
            assert got.dtype == np.uint8 and got.shape == (x.shape[0], yuv.frame_bytes(h, w, 8, chroma))
            for p, key in zip(yuv.split_planes(got, h, w, 8, chroma), ("y", "cb", "cr")):
                ref = gold[f"out/{chroma}/{h}x{w}/{key}"]
                assert ref.dtype == np.float64 and ref.shape == p.shape
                tie = np.abs(ref - np.floor(ref) - 0.5) <= TIE_EPS
                diff = np.abs(p.astype(np.float64) - np.rint(ref))
                assert (diff[~tie] == 0).all(), (chroma, h, w, key, float(diff[~tie].max()))
                assert (diff[tie] <= 1).all(), (chroma, h, w, key)
                near += int(tie.sum())
                total += tie.size
    print("near a tie:", near, "of", total)
    assert near <= 1e-3 * total


# ------------------------------------------------------------------------------------- bit for bit against the pinned 4:2:0 code
def _cases():
    return [(d, c) for d in DEPTHS for c in _colours(d)]


@pytest.mark.parametrize("depth,colour", _cases())
@pytest.mark.parametrize("h,w", [(2, 2), (3, 5), (8, 10), (9, 14)])
def test_replicated_chroma_gives_the_420_frames_rgb(depth, colour, h, w):
    fr = _frames(3, h, w, depth, "420", seed=h * w + depth)
    ref = yuv.i420_to_rgb(fr, h, w, colour, depth)
    for chroma in LAYOUTS:
        got = yuv.i420_to_rgb(replicated(fr, h, w, depth, chroma), h, w, colour, depth, chroma)
        assert got.dtype == np.float32 and got.tobytes() == ref.tobytes(), chroma


@pytest.mark.parametrize("depth,colour", _cases())
@pytest.mark.parametrize("H,W", [(2, 2), (3, 5), (8, 10), (9, 14)])
def test_luma_is_the_same_in_every_layout_and_block_constant_chroma_subsamples_to_420s(depth, colour, H, W):
    rng = np.random.RandomState(H + W + depth)
    x = rng.uniform(-0.25, 1.25, size=(2, 3, H, W)).astype(np.float32)
    y420 = yuv.split_planes(yuv.rgb_to_i420(x, colour, depth), H, W, depth)[0]
    for chroma in LAYOUTS:
        assert np.array_equal(yuv.split_planes(yuv.rgb_to_i420(x, colour, depth, chroma), H, W, depth, chroma)[0], y420)
    # constant over aligned 2 x 2 blocks: every block mean is one of its pixels, so the three layouts hold the same chroma
    ch, cw = yuv.chroma_hw(H, W)
    b = rng.uniform(-0.25, 1.25, size=(2, 3, ch, cw)).astype(np.float32)
    xb = np.repeat(np.repeat(b, 2, 2), 2, 3)[:, :, :H, :W].copy()
    _, u0, v0 = yuv.split_planes(yuv.rgb_to_i420(xb, colour, depth), H, W, depth)
    _, u2, v2 = yuv.split_planes(yuv.rgb_to_i420(xb, colour, depth, "422"), H, W, depth, "422")
    _, u4, v4 = yuv.split_planes(yuv.rgb_to_i420(xb, colour, depth, "444"), H, W, depth, "444")
    assert np.array_equal(u2[:, ::2], u0) and np.array_equal(v2[:, ::2], v0)
    assert np.array_equal(u4[:, ::2, ::2], u0) and np.array_equal(v4[:, ::2, ::2], v0)


def test_the_422_pair_and_the_odd_last_column():
    """(a + b) * 0.5 for a pair and the pixel alone in the last column of an odd W; 4:4:4 takes the pixel's own clamped RGB."""
    x = np.random.RandomState(1).uniform(-0.2, 1.2, size=(1, 3, 2, 5)).astype(np.float32)
    p = np.fmin(np.fmax(x, np.float32(0)), np.float32(1))
    _, cb, cr = yuv.ycbcr_f32(x, "bt601", "422")
    assert cb.shape == cr.shape == (1, 2, 3)
    t = yuv.BT601["to_ycbcr"]
    for j, m in enumerate([(p[:, :, :, 0] + p[:, :, :, 1]) * np.float32(0.5), (p[:, :, :, 2] + p[:, :, :, 3]) * np.float32(0.5), p[:, :, :, 4]]):
        assert np.array_equal(cb[:, :, j], yuv._row(m, t["cb"], 128.0)) and np.array_equal(cr[:, :, j], yuv._row(m, t["cr"], 128.0))
    _, cb4, _ = yuv.ycbcr_f32(x, "bt601", "444")
    assert np.array_equal(cb4, yuv._row(p, t["cb"], 128.0))


def test_pair_sad_takes_the_y_plane_of_every_layout():
    h, w = 5, 7
    for depth in (8, 10):
        v = _frames(4, h, w, depth, "420", seed=depth)
        ref = scenes.pair_sad(v, "i420", (h, w), depth)
        for chroma in LAYOUTS:
            fr = replicated(v, h, w, depth, chroma)
            assert np.array_equal(scenes.pair_sad(fr, "i" + chroma, (h, w), depth), ref)
            assert scenes.sad_samples(fr.shape, "i" + chroma, (h, w)) == h * w
    with pytest.raises(ValueError, match=r"I444 frames of 5 x 7 are \[N, 105\] uint8"):
        scenes.pair_sad(np.zeros((2, 59), np.uint8), "i444", (h, w))


# ------------------------------------------------------------------------------------------------------------------------------ Y4M
def _tag(chroma, depth):
    return ("420jpeg" if chroma == "420" else chroma) if depth == 8 else f"{chroma}p{depth}"


@pytest.mark.parametrize("chroma", ALL)
@pytest.mark.parametrize("depth", DEPTHS)
def test_y4m_round_trip_of_every_layout_and_depth(chroma, depth):
    h, w = 3, 5
    fr = _frames(5, h, w, depth, chroma, seed=depth)
    f = io.BytesIO()
    wr = y4m.Y4MWriter(f, w, h, fps=(30000, 1001), aspect=(4, 3), depth=depth, chroma=chroma)
    wr.write(fr[:2])
    wr.write(fr[2:])
    data = f.getvalue()
    assert data.startswith(f"YUV4MPEG2 W{w} H{h} F30000:1001 Ip A4:3 C{_tag(chroma, depth)}\n".encode())
    assert wr.frame_bytes == yuv.frame_bytes(h, w, depth, chroma) and len(data) == len(wr.header) + 5 * (6 + wr.frame_bytes)
    rd = y4m.Y4MReader(io.BytesIO(data), high_depth=True, layouts=ALL)
    assert (rd.chroma, rd.depth, rd.width, rd.height, rd.frame_bytes) == (chroma, depth, w, h, wr.frame_bytes)
    chunks = list(rd.chunks(2))
    assert [c.shape for c in chunks] == [(2, wr.frame_bytes)] * 2 + [(1, wr.frame_bytes)]
    assert np.array_equal(np.concatenate(chunks), fr)
    with pytest.raises(ValueError, match=r"\[m, %d\] uint8" % wr.frame_bytes):
        wr.write(fr[:, :-1])
    # the same stream through a pipe, in chunks that do not divide its length
    r, wfd = os.pipe()
    t = threading.Thread(target=lambda: os.fdopen(wfd, "wb").write(data))
    t.start()
    with os.fdopen(r, "rb", buffering=0) as pipe:
        got = np.concatenate(list(y4m.Y4MReader(pipe, high_depth=True, layouts=ALL).chunks(3)))
    t.join()
    assert np.array_equal(got, fr)


def test_y4m_default_reader_refuses_as_before_and_other_tags_stay_refused_by_name():
    for tag in ("C422", "C444", "C422p10"):
        with pytest.raises(ValueError, match=rf"colour space tag '{tag}' is not supported: 8-bit 4:2:0 only \(C420, C420jpeg, C420mpeg2, C420paldv\)"):
            y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4 " + tag.encode() + b"\n"))
        with pytest.raises(ValueError, match=f"colour space tag '{tag}' is not supported: 4:2:0 at 8, 10 or 12 bits only"):
            y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4 " + tag.encode() + b"\n"), high_depth=True)
    # 8-bit layouts without high_depth: the high-depth tags stay an opt-in of their own
    assert y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4 C444\n"), layouts=ALL).chroma == "444"
    with pytest.raises(ValueError, match=r"'C422p10' is not supported: 4:2:0, 4:2:2, 4:4:4 at 8 bits only \(.*C422, C444\)"):
        y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4 C422p10\n"), layouts=ALL)
    with pytest.raises(ValueError, match=r"'C444' is not supported: 4:2:0, 4:2:2 at 8 bits only \(C420, C420jpeg, C420mpeg2, C420paldv, C422\)"):
        y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4 C444\n"), layouts=("420", "422"))
    for tag in ("C444alpha", "Cmono", "C411", "C422p14", "C444p16"):
        with pytest.raises(ValueError, match=rf"colour space tag '{tag}' is not supported: 4:2:0, 4:2:2, 4:4:4 at 8, 10 or 12 bits only \(.*C444p12\)"):
            y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4 " + tag.encode() + b"\n"), high_depth=True, layouts=ALL)
    for tag in ("C420jpeg", "C420", "C420p10"):
        rd = y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4 " + tag.encode() + b"\n"), high_depth=True, layouts=ALL)
        assert rd.chroma == "420" and rd.frame_bytes == yuv.i420_bytes(4, 4, rd.depth)
    with pytest.raises(ValueError, match="layouts = '411': one of 420, 422, 444"):
        y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4\n"), layouts=("420", "411"))
    with pytest.raises(ValueError, match="y4m: chroma = '411': one of 420, 422, 444"):
        y4m.Y4MWriter(io.BytesIO(), 4, 4, chroma="411")


def test_y4m_truncated_422_frame_names_the_frame_and_both_byte_counts():
    h, w = 3, 5
    f = io.BytesIO()
    y4m.Y4MWriter(f, w, h, chroma="422").write(_frames(2, h, w, 8, "422"))
    rd = y4m.Y4MReader(io.BytesIO(f.getvalue()[:-7]), layouts=ALL)
    with pytest.raises(ValueError, match="y4m: frame 1 is truncated: 26 of 33 bytes"):
        list(rd.chunks(4))


def test_y4m_420_writer_headers_are_unchanged():
    a, b, c = io.BytesIO(), io.BytesIO(), io.BytesIO()
    y4m.Y4MWriter(a, 6, 4)
    y4m.Y4MWriter(b, 6, 4, chroma="420")
    y4m.Y4MWriter(c, 6, 4, depth=10, chroma="420")
    assert a.getvalue() == b.getvalue() == b"YUV4MPEG2 W6 H4 F25:1 Ip A0:0 C420jpeg\n"
    assert c.getvalue() == b"YUV4MPEG2 W6 H4 F25:1 Ip A0:0 C420p10\n"


# --------------------------------------------------------------------------------------------------------------------- the arguments
@pytest.fixture(scope="module")
def net():
    from savsr_amd.archs.savsr_arch import SAVSR
    return SAVSR().eval()


def _refused(net, match, frames=None, **kw):
    """upscale_video and VideoUpscaler refuse alike, on the host (the network is on the CPU: nothing can run)."""
    from savsr_amd import VideoUpscaler
    h, w = 8, 10
    fmt = kw.get("pixel_format", "rgb")
    if frames is None:
        frames = torch.zeros(9, yuv.frame_bytes(h, w, kw.get("depth", 8), fmt[1:]), dtype=torch.uint8) if fmt in ("i420", "i422", "i444") \
            else torch.zeros(9, h, w, 3, dtype=torch.uint8)
    if fmt != "rgb":
        kw.setdefault("size", (h, w))
    with pytest.raises(ValueError, match=match):
        net.upscale_video(frames, scale=2, **kw)
    with pytest.raises(ValueError, match=match):
        VideoUpscaler(net, 2, **kw)


def test_the_new_formats_are_appended_to_the_lists():
    from savsr_amd import video
    assert video.PIXEL_FORMATS == ("rgb", "i420", "i422", "i444") and video.OUT_KINDS == ("float", "uint8", "i420", "i422", "i444")


def test_arguments_of_the_new_formats_are_checked_by_name(net):
    _refused(net, "pixel_format = 'i411': one of rgb, i420, i422, i444", pixel_format="i411")
    _refused(net, "out = 'i440': one of float, uint8, i420, i422, i444", out="i440")
    _refused(net, r"pixel_format = 'i422' needs size = \(h, w\), got None", pixel_format="i422", size=None,
             frames=torch.zeros(9, 160, dtype=torch.uint8))
    _refused(net, "depth = 10 with colour = 'bt601-full': 10 and 12 bits are defined for limited range only",
             pixel_format="i444", depth=10, colour="bt601-full")
    _refused(net, "out_depth = 12 with out_colour = 'bt709-full': 10 and 12 bits are defined for limited range only",
             out="i422", out_depth=12, out_colour="bt709-full")
    _refused(net, "out_colour = 'bt709' goes with out = 'i420', 'i422' or 'i444'", pixel_format="i444", out_colour="bt709")
    _refused(net, "depth = 10 goes with pixel_format = 'i420', 'i422' or 'i444'", depth=10, out="i444")
    # accepted on the host: every pair of sides, the keywords of I420 on the new formats (the CPU network is what stops the call)
    for kw in (dict(pixel_format="i420", out="i444"), dict(out="i422"), dict(pixel_format="i422", depth=10, out="i444", out_depth=12),
               dict(pixel_format="i444", colour="bt709-full", out="i422", out_colour="bt601")):
        fmt = kw.get("pixel_format", "rgb")
        frames = torch.zeros(9, 8, 10, 3, dtype=torch.uint8) if fmt == "rgb" else \
            torch.zeros(9, yuv.frame_bytes(8, 10, kw.get("depth", 8), fmt[1:]), dtype=torch.uint8)
        with pytest.raises(RuntimeError, match="move the network to the GPU"):
            net.upscale_video(frames, scale=2, size=None if fmt == "rgb" else (8, 10), **kw)


def test_frames_of_the_new_formats_are_checked_naming_the_layout_and_the_byte_count(net):
    h, w = 8, 10
    with pytest.raises(ValueError, match="I422 frames of 8 x 10 have 160 bytes, got 120"):
        net.upscale_video(torch.zeros(9, 120, dtype=torch.uint8), scale=2, pixel_format="i422", size=(h, w))
    with pytest.raises(ValueError, match=r"10-bit I444 frames of 8 x 10 have 480 bytes \(16-bit samples\), got 240"):
        net.upscale_video(torch.zeros(9, 240, dtype=torch.uint8), scale=2, pixel_format="i444", size=(h, w), depth=10)
    with pytest.raises(ValueError, match="I444 frames must be uint8"):
        net.upscale_video(torch.zeros(9, 240, dtype=torch.int16), scale=2, pixel_format="i444", size=(h, w))
    fb = yuv.frame_bytes(h, w, 12, "422")
    raw = torch.zeros(9 * fb + 2, dtype=torch.uint8)
    odd = raw[1 + raw.data_ptr() % 2:][:9 * fb].view(9, fb)
    assert odd.data_ptr() % 2 == 1
    with pytest.raises(ValueError, match="12-bit I422 frames hold 16-bit samples: the base pointer 0x[0-9a-f]+ is not 2-byte aligned"):
        net.upscale_video(odd, scale=2, pixel_format="i422", size=(h, w), depth=12)


def test_cli_out_chroma_is_parsed_and_goes_with_a_y4m_output(capsys):
    from savsr_amd.upscale import parse_args
    base = ["--scale", "2", "--checkpoint", "x.pth"]
    assert parse_args(["-i", "a.y4m", "-o", "b.y4m"] + base).out_chroma is None
    assert parse_args(["-i", "a.y4m", "-o", "b.y4m", "--out-chroma", "same"] + base).out_chroma is None
    assert parse_args(["-i", "lr", "-o", "b.y4m", "--out-chroma", "444"] + base).out_chroma == "444"
    assert parse_args(["-i", "a.y4m", "-o", "-", "--out-chroma", "422", "--out-depth", "10"] + base).out_chroma == "422"
    with pytest.raises(SystemExit):
        parse_args(["-i", "a.y4m", "-o", "sr", "--out-chroma", "444"] + base)
    assert "--out-chroma goes with a Y4M output" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(["-i", "a.y4m", "-o", "b.y4m", "--out-chroma", "411"] + base)


def test_cli_refuses_full_range_at_high_depth_on_a_422_input_before_anything_runs(net, tmp_path):
    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    ckpt, src = tmp_path / "net.pth", tmp_path / "full422p10.y4m"
    sio.save_network(net, str(ckpt))
    with open(src, "wb") as f:
        y4m.Y4MWriter(f, 10, 8, colour_range="full", depth=10, chroma="422").write(_frames(9, 8, 10, 10, "422"))
    with pytest.raises(SystemExit, match="depth = 10 with colour = 'bt601-full': 10 and 12 bits are defined for limited range only"):
        main(["-i", str(src), "-o", str(tmp_path / "a.y4m"), "--colour", "auto", "--scale", "2", "--checkpoint", str(ckpt), "--device", "cpu"])
    assert not (tmp_path / "a.y4m").exists()
