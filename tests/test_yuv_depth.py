"""10- and 12-bit YUV 4:2:0 without a GPU: the high-depth half of savsr_amd/yuv.py (the restatement savsr_video_gather_yuv420_16 /
savsr_video_quantize_yuv420_16 are tested against) pinned by the float64 closed form and by the 8-bit path, scenes.pair_sad with depth=,
the Y4M reader / writer at C420p10 / C420p12 and the refusals of depth / out_depth (all of them raise before the GPU is touched)."""
import io

import numpy as np
import pytest
import torch

from savsr_amd import scenes, y4m, yuv

DEPTHS = (10, 12)
LIMITED = ("bt601", "bt709")
# i420_to_rgb at 10 / 12 bits makes at most five float32 roundings of values below 2.5 (two products, two sums and the offset's own
# rounding on R and B; G's terms are smaller): 5 * 2.5 * 2^-24 = 7.5e-7 < 1e-6 from the float64 closed form.
BOUND = 1e-6


def _frame16(y, u, v):
    """Planes (uint16 arrays [h, w], [ch, cw], [ch, cw]) -> one high-depth frame [1, bytes] uint8."""
    return np.concatenate([np.asarray(p, "<u2").reshape(-1) for p in (y, u, v)]).view(np.uint8)[None]


def _closed_form(y, u, v, colour, depth):
    """float64: the colour space's ycbcr2rgb on samples / k, clamped; y, u, v broadcastable sample arrays."""
    t = yuv.matrix(colour)["to_rgb"]
    k = float(1 << (depth - 8))
    y, u, v = (np.asarray(p, np.float64) / k for p in (y, u, v))
    o = [c / 255.0 for c in t["offset"]]
    rgb = np.stack(np.broadcast_arrays(y * t["y"] + v * t["rv"] + o[0], y * t["y"] + u * t["gu"] + v * t["gv"] + o[1], y * t["y"] + u * t["bu"] + o[2]))
    return np.clip(rgb, 0.0, 1.0)


def _convert_pixels(y, u, v, colour, depth):
    """i420_to_rgb on a list of (y, u, v) triples: one 2 x 2 frame per triple (the block shares its chroma) -> [3, n] of pixel (0, 0)."""
    n = len(y)
    fr = np.empty((n, 6), "<u2")
    fr[:, :4] = np.asarray(y)[:, None]
    fr[:, 4] = u
    fr[:, 5] = v
    rgb = yuv.i420_to_rgb(fr.view(np.uint8), 2, 2, colour, depth)
    assert rgb.dtype == np.float32 and rgb.shape == (n, 3, 2, 2)
    assert np.array_equal(rgb, np.broadcast_to(rgb[:, :, :1, :1], rgb.shape))         # chroma replicated over the block
    return rgb[:, :, 0, 0].T


@pytest.mark.parametrize("colour", LIMITED)
@pytest.mark.parametrize("depth", DEPTHS)
def test_i420_to_rgb_within_the_derived_bound_of_the_float64_closed_form(colour, depth):
    top, mid = (1 << depth) - 1, 1 << (depth - 1)
    codes = np.arange(top + 1)
    rng = np.random.RandomState(depth)
    tri = rng.randint(0, top + 1, size=(10 ** 4, 3))
    for name, (y, u, v) in {"every Y code at neutral chroma": (codes, np.full_like(codes, mid), np.full_like(codes, mid)),
                            "every Cb code at mid grey": (np.full_like(codes, mid), codes, np.full_like(codes, mid)),
                            "every Cr code at mid grey": (np.full_like(codes, mid), np.full_like(codes, mid), codes),
                            "random triples": (tri[:, 0], tri[:, 1], tri[:, 2])}.items():
        got = _convert_pixels(y, u, v, colour, depth)
        err = float(np.abs(got.astype(np.float64) - _closed_form(y, u, v, colour, depth)).max())
        print(colour, depth, name, "max-abs", err)
        assert err <= BOUND, name
        assert got.min() >= 0.0 and got.max() <= 1.0


@pytest.mark.parametrize("colour", LIMITED)
@pytest.mark.parametrize("h,w", [(2, 2), (3, 5), (16, 48)])
def test_scaled_samples_of_an_8_bit_frame_give_the_8_bit_rgb(colour, h, w):
    fr8 = (np.arange(3 * yuv.i420_bytes(h, w)) * 7 % 256).astype(np.uint8).reshape(3, -1)
    ref = yuv.i420_to_rgb(fr8, h, w, colour)
    for depth in DEPTHS:
        fr = (fr8.astype("<u2") << (depth - 8)).view(np.uint8)
        assert fr.shape == (3, yuv.i420_bytes(h, w, depth)) == (3, 2 * yuv.i420_bytes(h, w))
        got = yuv.i420_to_rgb(fr, h, w, colour, depth)
        err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
        print(colour, depth, (h, w), "max-abs", err)
        assert err <= BOUND


@pytest.mark.parametrize("depth", DEPTHS)
def test_samples_above_the_depth_read_as_its_largest_code(depth):
    top = (1 << depth) - 1
    y = np.array([[top + 1, 0xffff], [top, 1 << depth]], np.uint16)
    over = _frame16(y, [[0xffff]], [[top + 7]])
    capped = _frame16(np.minimum(y, top), [[top]], [[top]])
    assert np.array_equal(yuv.i420_to_rgb(over, 2, 2, "bt709", depth), yuv.i420_to_rgb(capped, 2, 2, "bt709", depth))
    vid = np.concatenate([over, capped, _frame16(np.zeros((2, 2)), [[0]], [[0]])])
    assert scenes.pair_sad(vid, "i420", (2, 2), depth).tolist() == [0, 4 * 255]


def test_frame_layout_at_high_depth():
    assert yuv.i420_bytes(3, 5, 8) == 27 and yuv.i420_bytes(3, 5, 10) == 54 and yuv.i420_bytes(3, 5, 12) == 54
    fr = np.arange(27, dtype="<u2").view(np.uint8)[None]
    y, u, v = yuv.split_planes(fr, 3, 5, 10)
    assert y.dtype == np.uint16 and y.shape == (1, 3, 5) and u.shape == (1, 2, 3) and v.shape == (1, 2, 3)
    assert y[0, 2, 4] == 14 and u[0, 0, 0] == 15 and v[0, 1, 2] == 26
    assert fr[0, 0] == 0 and fr[0, 2] == 1 and fr[0, 3] == 0                            # little-endian
    with pytest.raises(ValueError, match=r"10-bit I420 frames of 3 x 5 are \[N, 54\] uint8"):
        yuv.split_planes(fr[:, :27], 3, 5, 10)


@pytest.mark.parametrize("colour", LIMITED)
@pytest.mark.parametrize("depth", DEPTHS)
def test_rgb_to_i420_is_the_rounded_scaled_float32_value(colour, depth):
    k = 1 << (depth - 8)
    rng = np.random.RandomState(depth)
    for h, w in [(2, 2), (3, 5), (9, 14)]:
        x = rng.uniform(-0.25, 1.25, size=(2, 3, h, w)).astype(np.float32)
        x[0, :, 0, 0] = np.nan
        got = yuv.rgb_to_i420(x, colour, depth)
        assert got.dtype == np.uint8 and got.shape == (2, yuv.i420_bytes(h, w, depth))
        for p, f in zip(yuv.split_planes(got, h, w, depth), yuv.ycbcr_f32(x, colour)):
            assert p.dtype == np.uint16 and p.shape == f.shape
            assert (np.abs(p.astype(np.float64) / k - f.astype(np.float64)) <= 0.5 / k).all()          # exact: both sides are dyadic
        y = yuv.split_planes(got, h, w, depth)[0]
        assert y[0, 0, 0] == 16 * k                                                     # NaN -> 0 after the clamp: black
    x = rng.uniform(0, 1, size=(2, 3, 5, 7)).astype(np.float32)
    assert np.array_equal(yuv.rgb_to_i420(x, colour, 8), yuv.rgb_to_i420(x, colour))     # depth = 8: today's function, byte for byte
    assert yuv.rgb_to_i420(x, colour, 8).tobytes() == yuv.rgb_to_i420(x, colour).tobytes()


def grey_ties(colour, depth):
    """Grey levels g (float32) on which the float32 Y of the restatement, times k, is exactly n + 0.5: searched among the float32
    neighbours of the level that would give it in exact arithmetic.  {n: g}"""
    k = 1 << (depth - 8)
    found = {}
    for n in range(16 * k, 235 * k, 1 if k == 4 else 5):                   # (an odd stride: both parities)
        g0 = np.float32(((n + 0.5) / k - 16.0) / 219.0)
        cand = [g0]
        for _ in range(48):
            cand.append(np.nextafter(cand[-1], np.float32(2.0)))
        lo = g0
        for _ in range(48):
            lo = np.nextafter(lo, np.float32(-1.0))
            cand.append(lo)
        cand = np.array(cand, np.float32)
        img = np.broadcast_to(cand[None, None, None, :], (1, 3, 2, cand.size)).copy()
        y = yuv.ycbcr_f32(img, colour)[0][0, 0] * np.float32(k)
        hit = np.nonzero(y == np.float32(n + 0.5))[0]
        if hit.size:
            found[n] = cand[hit[0]]
    return found


@pytest.mark.parametrize("depth", DEPTHS)
def test_rgb_to_i420_ties_round_to_even(depth):
    ties = grey_ties("bt601", depth)
    assert len(ties) >= 100, len(ties)
    ns = sorted(ties)
    assert any(n % 2 for n in ns) and any(n % 2 == 0 for n in ns)
    img = np.broadcast_to(np.array([ties[n] for n in ns], np.float32)[None, None, None, :], (1, 3, 2, len(ns))).copy()
    y = yuv.split_planes(yuv.rgb_to_i420(img, "bt601", depth), 2, len(ns), depth)[0][0, 0]
    assert np.array_equal(y, np.array([n if n % 2 == 0 else n + 1 for n in ns], np.uint16))


@pytest.mark.parametrize("colour", LIMITED)
@pytest.mark.parametrize("depth", DEPTHS)
def test_rgb_to_i420_range_on_the_gamut_corners(colour, depth):
    k = 1 << (depth - 8)
    c = np.array([-5.0, 0.0, 1.0, 7.0], np.float32)
    img = np.stack(np.meshgrid(c, c, c, indexing="ij"), 0).reshape(3, 8, 8)[None]
    corners = np.repeat(np.repeat(img, 2, 2), 2, 3)                                      # every corner fills a whole chroma block
    y, u, v = yuv.split_planes(yuv.rgb_to_i420(corners, colour, depth), 16, 16, depth)
    assert y.min() == 16 * k and y.max() == 235 * k
    assert min(u.min(), v.min()) == 16 * k and max(u.max(), v.max()) == 240 * k
    assert np.array_equal(yuv.rgb_to_i420(corners, colour, depth), yuv.rgb_to_i420(np.clip(corners, 0, 1), colour, depth))


@pytest.mark.parametrize("colour", LIMITED)
def test_round_trip_is_the_identity_on_the_10_bit_grey_axis(colour):
    codes = np.arange(64, 941)                                                          # 16 k .. 235 k: the in-gamut greys
    fr = np.empty((codes.size, 6), "<u2")
    fr[:, :4] = codes[:, None]
    fr[:, 4:] = 512
    fr = fr.view(np.uint8)
    rgb = yuv.i420_to_rgb(fr, 2, 2, colour, 10)
    assert np.array_equal(yuv.rgb_to_i420(rgb, colour, 10), fr)


# ------------------------------------------------------------------------------------------------------------------------------ Y4M
def _frames16(n, h, w, depth, seed=0):
    s = np.random.RandomState(seed).randint(0, 1 << depth, size=(n, yuv.i420_bytes(h, w)))
    return s.astype("<u2").view(np.uint8)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("h,w", [(3, 5), (4, 6), (2, 2)])
def test_y4m_round_trip_at_high_depth(depth, h, w):
    fr = _frames16(5, h, w, depth, seed=h)
    f = io.BytesIO()
    wr = y4m.Y4MWriter(f, w, h, fps=(30000, 1001), aspect=(4, 3), depth=depth)
    wr.write(fr[:2])
    wr.write(fr[2:])
    data = f.getvalue()
    assert data.startswith(f"YUV4MPEG2 W{w} H{h} F30000:1001 Ip A4:3 C420p{depth}\n".encode())
    assert wr.frame_bytes == 2 * yuv.i420_bytes(h, w) and len(data) == len(wr.header) + 5 * (6 + wr.frame_bytes)
    rd = y4m.Y4MReader(io.BytesIO(data), high_depth=True)
    assert (rd.depth, rd.width, rd.height, rd.colorspace, rd.frame_bytes) == (depth, w, h, f"420p{depth}", wr.frame_bytes)
    chunks = list(rd.chunks(2))
    assert [c.shape for c in chunks] == [(2, wr.frame_bytes), (2, wr.frame_bytes), (1, wr.frame_bytes)] and chunks[0].dtype == np.uint8
    assert np.array_equal(np.concatenate(chunks), fr)
    with pytest.raises(ValueError, match=r"\[m, %d\] uint8" % wr.frame_bytes):
        wr.write(fr[:, :yuv.i420_bytes(h, w)])


def test_y4m_writer_depth_8_writes_todays_header_and_bad_depths_are_refused():
    a, b = io.BytesIO(), io.BytesIO()
    y4m.Y4MWriter(a, 6, 4)
    y4m.Y4MWriter(b, 6, 4, depth=8)
    assert a.getvalue() == b.getvalue() == b"YUV4MPEG2 W6 H4 F25:1 Ip A0:0 C420jpeg\n"
    for bad in (9, 14, 16, "10"):
        with pytest.raises(ValueError, match="y4m: depth = .*: one of 8, 10, 12"):
            y4m.Y4MWriter(io.BytesIO(), 6, 4, depth=bad)


def test_y4m_reader_high_depth_is_an_opt_in_and_other_tags_stay_refused():
    hdr = b"YUV4MPEG2 W4 H4 F25:1 C420p10\n"
    with pytest.raises(ValueError, match=r"colour space tag 'C420p10' is not supported: 8-bit 4:2:0 only \(C420, C420jpeg, C420mpeg2, C420paldv\)"):
        y4m.Y4MReader(io.BytesIO(hdr))
    assert y4m.Y4MReader(io.BytesIO(hdr), high_depth=True).depth == 10
    for tag in ("C420jpeg", "C420", "C420mpeg2", "C420paldv"):
        rd = y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4 " + tag.encode() + b"\n"), high_depth=True)
        assert rd.depth == 8 and rd.frame_bytes == yuv.i420_bytes(4, 4)
    assert y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4\n"), high_depth=True).depth == 8
    for tag in ("C422", "C444", "C420p14", "C420p16", "C422p10", "Cmono"):
        with pytest.raises(ValueError, match=f"colour space tag '{tag}' is not supported: 4:2:0 at 8, 10 or 12 bits only"):
            y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4 " + tag.encode() + b"\n"), high_depth=True)


def test_y4m_truncated_high_depth_frame_names_the_frame_and_the_byte_counts():
    h, w = 3, 5
    fr = _frames16(2, h, w, 10)
    f = io.BytesIO()
    y4m.Y4MWriter(f, w, h, depth=10).write(fr)
    rd = y4m.Y4MReader(io.BytesIO(f.getvalue()[:-7]), high_depth=True)
    with pytest.raises(ValueError, match="y4m: frame 1 is truncated: 47 of 54 bytes"):
        list(rd.chunks(4))


# --------------------------------------------------------------------------------------------------------------------- the arguments
@pytest.fixture(scope="module")
def net():
    from savsr_amd.archs.savsr_arch import SAVSR
    return SAVSR().eval()


def _refused(net, match, frames=None, **kw):
    """upscale_video and VideoUpscaler refuse alike, on the host (the network is on the CPU: nothing can run)."""
    from savsr_amd import VideoUpscaler
    h, w = 8, 10
    if frames is None:
        frames = torch.zeros(9, yuv.i420_bytes(h, w, kw.get("depth", 8)), dtype=torch.uint8) if kw.get("pixel_format") == "i420" \
            else torch.zeros(9, h, w, 3, dtype=torch.uint8)
    if kw.get("pixel_format") == "i420":
        kw.setdefault("size", (h, w))
    with pytest.raises(ValueError, match=match):
        net.upscale_video(frames, scale=2, **kw)
    with pytest.raises(ValueError, match=match):
        VideoUpscaler(net, 2, **kw)


def test_depth_arguments_are_checked_by_name(net):
    for bad in (9, 14, 16, "10", 10.0, None, True):
        _refused(net, "depth = .*: one of 8, 10, 12", pixel_format="i420", depth=bad)
    for bad in (9, 14, "12", 12.0):
        _refused(net, "out_depth = .*: one of 8, 10, 12", out="i420", out_depth=bad)
    _refused(net, "depth = 10 goes with pixel_format = 'i420'", depth=10)
    _refused(net, "out_depth = 10 goes with out = 'i420'", out_depth=10)
    _refused(net, "out_depth = 8 goes with out = 'i420'", out="uint8", out_depth=8)
    _refused(net, "out_depth = 12 goes with out = 'i420'", pixel_format="i420", depth=12, out="float", out_depth=12)
    _refused(net, "depth = 10 with colour = 'bt601-full': 10 and 12 bits are defined for limited range only",
             pixel_format="i420", depth=10, colour="bt601-full")
    _refused(net, "out_depth = 12 with out_colour = 'bt709-full': 10 and 12 bits are defined for limited range only",
             out="i420", out_depth=12, out_colour="bt709-full")
    # out_colour = None is the input's colour space, out_depth = None the input's depth
    _refused(net, "out_depth = 10 with out_colour = 'bt709-full'", pixel_format="i420", colour="bt709-full", out="i420", out_depth=10)
    _refused(net, "out_depth = 10 with out_colour = 'bt601-full'", pixel_format="i420", depth=10, out="i420", out_colour="bt601-full")
    # the pinned refusals of the names are untouched
    _refused(net, "pixel_format = 'nv12': one of rgb, i420", pixel_format="nv12", depth=10)
    _refused(net, "out = 'yuv': one of float, uint8, i420", out="yuv", out_depth=10)


def test_high_depth_frames_are_checked(net):
    h, w = 8, 10
    with pytest.raises(ValueError, match=r"10-bit I420 frames of 8 x 10 have 240 bytes \(16-bit samples\), got 120"):
        net.upscale_video(torch.zeros(9, yuv.i420_bytes(h, w), dtype=torch.uint8), scale=2, pixel_format="i420", size=(h, w), depth=10)
    with pytest.raises(ValueError, match="I420 frames must be uint8"):
        net.upscale_video(torch.zeros(9, yuv.i420_bytes(h, w), dtype=torch.int16), scale=2, pixel_format="i420", size=(h, w), depth=10)
    fb = yuv.i420_bytes(h, w, 12)
    raw = torch.zeros(9 * fb + 1, dtype=torch.uint8)
    odd = raw[1 - raw.data_ptr() % 2:][:9 * fb].view(9, fb)
    if odd.data_ptr() % 2 == 0:
        odd = raw[1:].view(9, fb)
    assert odd.data_ptr() % 2 == 1
    with pytest.raises(ValueError, match="12-bit I420 frames hold 16-bit samples: the base pointer 0x[0-9a-f]+ is not 2-byte aligned"):
        net.upscale_video(odd, scale=2, pixel_format="i420", size=(h, w), depth=12)


def test_yuv_module_refuses_full_range_at_high_depth():
    x = np.zeros((1, 3, 2, 2), np.float32)
    with pytest.raises(ValueError, match="depth = 10 with colour = 'bt709-full': 10 and 12 bits are defined for limited range only"):
        yuv.rgb_to_i420(x, "bt709-full", 10)
    with pytest.raises(ValueError, match="depth = 12 with colour = 'bt601-full'"):
        yuv.i420_to_rgb(np.zeros((1, 12), np.uint8), 2, 2, "bt601-full", 12)
    with pytest.raises(ValueError, match="depth = 9: one of 8, 10, 12"):
        yuv.rgb_to_i420(x, "bt601", 9)


# ------------------------------------------------------------------------------------------------------------------------ scene cuts
@pytest.mark.parametrize("depth", DEPTHS)
def test_pair_sad_of_scaled_samples_equals_the_8_bit_videos(depth):
    h, w = 5, 7
    rng = np.random.RandomState(depth)
    v8 = rng.randint(0, 256, size=(6, yuv.i420_bytes(h, w)), dtype=np.uint8)
    ref = scenes.pair_sad(v8, "i420", (h, w))
    low = rng.randint(0, 1 << (depth - 8), size=v8.shape)                               # the bits below the 8 most significant ones
    v16 = ((v8.astype("<u2") << (depth - 8)) | low.astype("<u2")).view(np.uint8)
    got = scenes.pair_sad(v16, "i420", (h, w), depth=depth)
    assert got.dtype == np.int64 and np.array_equal(got, ref)
    assert np.array_equal(scenes.pair_sad(torch.from_numpy(v16), "i420", (h, w), depth), ref)
    assert scenes.sad_samples(v16.shape, "i420", (h, w)) == h * w                        # the scale of the threshold is untouched
    with pytest.raises(ValueError, match="depth = 10 goes with pixel_format = 'i420'"):
        scenes.pair_sad(np.zeros((2, h, w, 3), np.uint8), depth=10)


# ------------------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_out_depth_is_parsed_and_goes_with_a_y4m_output(capsys):
    from savsr_amd.upscale import parse_args
    base = ["--scale", "2", "--checkpoint", "x.pth"]
    assert parse_args(["-i", "a.y4m", "-o", "b.y4m"] + base).out_depth is None
    assert parse_args(["-i", "a.y4m", "-o", "b.y4m", "--out-depth", "same"] + base).out_depth is None
    assert parse_args(["-i", "lr", "-o", "b.y4m", "--out-depth", "10"] + base).out_depth == 10
    assert parse_args(["-i", "a.y4m", "-o", "-", "--out-depth", "12"] + base).out_depth == 12
    with pytest.raises(SystemExit):
        parse_args(["-i", "a.y4m", "-o", "sr", "--out-depth", "10"] + base)
    assert "--out-depth goes with a Y4M output" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(["-i", "a.y4m", "-o", "b.y4m", "--out-depth", "9"] + base)


def test_cli_refuses_full_range_at_high_depth_before_anything_runs(net, tmp_path):
    """A C420p10 input tagged full range with --colour auto, and a full-range output with --out-depth 10: refused by the rule's name."""
    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    ckpt, src, src8 = tmp_path / "net.pth", tmp_path / "full10.y4m", tmp_path / "lr8.y4m"
    sio.save_network(net, str(ckpt))
    with open(src, "wb") as f:
        y4m.Y4MWriter(f, 10, 8, colour_range="full", depth=10).write(_frames16(9, 8, 10, 10))
    with open(src8, "wb") as f:
        y4m.Y4MWriter(f, 10, 8).write(np.zeros((9, yuv.i420_bytes(8, 10)), np.uint8))
    base = ["--scale", "2", "--checkpoint", str(ckpt), "--device", "cpu"]
    with pytest.raises(SystemExit, match="depth = 10 with colour = 'bt601-full': 10 and 12 bits are defined for limited range only"):
        main(["-i", str(src), "-o", str(tmp_path / "a.y4m"), "--colour", "auto"] + base)
    with pytest.raises(SystemExit, match="out_depth = 10 with out_colour = 'bt709-full'"):
        main(["-i", str(src8), "-o", str(tmp_path / "b.y4m"), "--out-colour", "bt709-full", "--out-depth", "10"] + base)
    assert not (tmp_path / "a.y4m").exists() and not (tmp_path / "b.y4m").exists()
