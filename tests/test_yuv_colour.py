"""The four colour spaces of the raw-video path on the host (savsr_amd/yuv.py `COLOURS` / `matrix`, the specification of
savsr_video_gather_yuv420 / savsr_video_quantize_yuv420): anchors from the standards, the grey axis, both directions against a float64
closed form written here from (Kr, Kb, range), exact round trips, the BT.601 -> BT.709 conversion, the defaults unchanged, the host-side
refusals, XCOLORRANGE in Y4M headers and the CLI's two flags with their `auto` rule."""
import io

import numpy as np
import pytest
import torch

from savsr_amd import y4m, yuv

SPACES = {"bt601": (0.299, 0.114, False), "bt709": (0.2126, 0.0722, False), "bt601-full": (0.299, 0.114, True),
          "bt709-full": (0.2126, 0.0722, True)}
SIZES = [(2, 2), (3, 5), (8, 12), (7, 12), (9, 11)]
TIE = 1e-4          # six float32 operations on values <= 255 err by at most ~1e-4 (half an ulp of 255 is 7.6e-6 per operation, the
#                     coefficients' own rounding 1.5e-5): a float64 value nearer than this to k + 0.5 may round either way in float32
TIE_SHARE = 0.005


def test_the_names_their_order_and_the_default_table():
    assert yuv.COLOURS == ("bt601", "bt709", "bt601-full", "bt709-full")          # the position is the id of the C ABI
    assert yuv.matrix("bt601") is yuv.BT601 and yuv.matrix() is yuv.BT601
    for c in yuv.COLOURS:
        m = yuv.matrix(c)
        assert set(m) == {"to_rgb", "to_ycbcr"} and set(m["to_rgb"]) == set(yuv.BT601["to_rgb"]) and set(m["to_ycbcr"]) == set(yuv.BT601["to_ycbcr"])
        assert len(m["to_rgb"]["offset"]) == 3 and all(len(m["to_ycbcr"][k]) == 3 for k in ("y", "cb", "cr", "offset"))
        assert yuv.matrix(c) is m                                                 # one table per name
    with pytest.raises(ValueError, match="colour = 'bt2020': one of bt601, bt709, bt601-full, bt709-full"):
        yuv.matrix("bt2020")
    with pytest.raises(ValueError, match="one of bt601, bt709, bt601-full, bt709-full"):
        yuv.rgb_to_i420(np.zeros((1, 3, 2, 2), np.float32), colour="BT709")


# ---------------------------------------------------------------------------------------------------------- float64 closed forms
def _scales(full):
    return (255.0, 0.0, 255.0) if full else (219.0, 16.0, 224.0)


def _rows64(colour):
    """rows [3][3] and offsets [3] of RGB in [0, 1] -> (Y, Cb, Cr) in 8-bit steps.  bt601 is the reference's own matrix (rounded
    constants, tests/test_yuv.py pins it to the reference); the others follow from (Kr, Kb, range)."""
    if colour == "bt601":
        t = yuv.BT601["to_ycbcr"]
        return np.array([t["y"], t["cb"], t["cr"]], np.float64), np.array(t["offset"], np.float64)
    kr, kb, full = SPACES[colour]
    kg = 1.0 - kr - kb
    sy, oy, sc = _scales(full)
    y = np.array([kr, kg, kb])
    cb = (np.array([0.0, 0.0, 1.0]) - y) / (2.0 * (1.0 - kb))
    cr = (np.array([1.0, 0.0, 0.0]) - y) / (2.0 * (1.0 - kr))
    return np.stack([sy * y, sc * cb, sc * cr]), np.array([oy, 128.0, 128.0])


def _to_rgb64(frames, h, w, colour):
    """float64 RGB [N, 3, h, w] of I420 frames, clamped to [0, 1]."""
    y, u, v = (p.astype(np.float64) for p in yuv.split_planes(frames, h, w))
    u, v = (np.repeat(np.repeat(p, 2, 1), 2, 2)[:, :h, :w] for p in (u, v))
    if colour == "bt601":
        t = yuv.BT601["to_rgb"]
        o = [x / 255.0 for x in t["offset"]]
        rgb = [y * t["y"] + v * t["rv"] + o[0], y * t["y"] + u * t["gu"] + v * t["gv"] + o[1], y * t["y"] + u * t["bu"] + o[2]]
    else:
        kr, kb, full = SPACES[colour]
        kg = 1.0 - kr - kb
        sy, oy, sc = _scales(full)
        yy, cb, cr = (y - oy) / sy, (u - 128.0) / sc, (v - 128.0) / sc
        r = yy + 2.0 * (1.0 - kr) * cr
        b = yy + 2.0 * (1.0 - kb) * cb
        rgb = [r, (yy - kr * r - kb * b) / kg, b]
    return np.clip(np.stack(rgb, 1), 0.0, 1.0)


def _block_mean64(p):
    n, c, H, W = p.shape
    ch, cw = yuv.chroma_hw(H, W)
    pad = np.full((n, c, 2 * ch, 2 * cw), np.nan)
    pad[:, :, :H, :W] = p
    return np.nanmean(pad.reshape(n, c, ch, 2, cw, 2), axis=(3, 5))


def _to_i420_64(x64, colour):
    """The float64 (Y, Cb, Cr) planes, flattened per frame as an I420 frame lies: what rgb_to_i420 rounds."""
    p = np.clip(x64, 0.0, 1.0)
    rows, off = _rows64(colour)
    n = p.shape[0]
    y = np.tensordot(rows[0], p, axes=([0], [1])) + off[0]
    m = _block_mean64(p)
    cb = np.tensordot(rows[1], m, axes=([0], [1])) + off[1]
    cr = np.tensordot(rows[2], m, axes=([0], [1])) + off[2]
    return np.concatenate([v.reshape(n, -1) for v in (y, cb, cr)], 1)


def _assert_rounds_to(pairs, colour):
    """Over all (got uint8, exact float64) pairs of a test: got == rint(exact), clipped for full range, but for samples within TIE of a
    half-integer: at most TIE_SHARE of them, off by <= 1."""
    got_u8 = np.concatenate([g.reshape(-1) for g, _ in pairs])
    exact64 = np.concatenate([e.reshape(-1) for _, e in pairs])
    want = np.rint(exact64)
    if SPACES[colour][2]:
        want = np.clip(want, 0, 255)
    near = np.abs(exact64 - np.floor(exact64) - 0.5) < TIE
    assert near.mean() <= TIE_SHARE, near.mean()
    diff = np.abs(got_u8.astype(np.int64) - want.astype(np.int64))
    assert not diff[~near].any(), (colour, int(diff[~near].max()), int((diff[~near] != 0).sum()))
    assert diff.max() <= 1


# ------------------------------------------------------------------------------------------------------------------------ anchors
@pytest.mark.parametrize("colour,rgb,want", [
    ("bt709", (1, 0, 0), (63, 102, 240)),
    ("bt709", (0, 1, 0), (173, 42, 26)),
    ("bt709", (0, 0, 1), (32, 240, 118)),
    ("bt709", (1, 1, 1), (235, 128, 128)),
    ("bt709", (0, 0, 0), (16, 128, 128)),
    ("bt601-full", (1, 0, 0), (76, 85, 255)),          # the clip case: Cr = 255.5 rounds to 256
    ("bt601-full", (1, 1, 1), (255, 128, 128)),
    ("bt709-full", (0, 0, 1), (18, 255, 116)),         # the clip case: Cb = 255.5
])
def test_anchors_from_the_standards(colour, rgb, want):
    x = np.broadcast_to(np.array(rgb, np.float32)[None, :, None, None], (1, 3, 2, 2)).copy()
    f = yuv.rgb_to_i420(x, colour=colour)
    assert f.shape == (1, 6) and f.dtype == np.uint8
    assert tuple(int(v) for v in f[0, :4]) == (want[0],) * 4
    assert (int(f[0, 4]), int(f[0, 5])) == want[1:]


def test_full_range_clip_acts_on_the_float_values():
    red = np.broadcast_to(np.array((1, 0, 0), np.float32)[None, :, None, None], (1, 3, 2, 2)).copy()
    assert float(yuv.ycbcr_f32(red, "bt601-full")[2][0, 0, 0]) == 255.5           # exactly representable: rint gives 256
    blue = red[:, ::-1].copy()
    assert float(yuv.ycbcr_f32(blue, "bt709-full")[1][0, 0, 0]) == 255.5


@pytest.mark.parametrize("colour", yuv.COLOURS)
def test_grey_axis(colour):
    """U = V = 128: R = G = B = (Y - 16) / 219, or Y / 255 at full range, within the float32 evaluation bound of this path (2e-6: three
    table roundings and two sums of values <= 1.2).  The three built matrices lie on the axis exactly in float64.  bt601's table is the
    reference's, kept as it is: its rounded constants leave the axis by themselves (2.4e-6 on R at Y = 235, computed below in float64
    from the constants alone), and that distance is added to the bound for bt601 only."""
    full = SPACES[colour][2]
    ys = np.arange(0, 256) if full else np.arange(16, 236)
    fr = np.full((len(ys), 6), 128, np.uint8)
    fr[:, :4] = ys[:, None]
    want = ys / 255.0 if full else (ys - 16.0) / 219.0
    t = yuv.matrix(colour)["to_rgb"]
    exact = np.stack([ys * t["y"] + 128 * t["rv"] + t["offset"][0] / 255.0, ys * t["y"] + 128 * (t["gu"] + t["gv"]) + t["offset"][1] / 255.0,
                      ys * t["y"] + 128 * t["bu"] + t["offset"][2] / 255.0], 1)
    off_axis = float(np.abs(exact - want[:, None]).max())
    if colour == "bt601":
        assert 2e-6 < off_axis < 3e-6                     # the reference's constants, not this code
    else:
        assert off_axis < 1e-15
        off_axis = 0.0
    rgb = yuv.i420_to_rgb(fr, 2, 2, colour=colour).astype(np.float64)
    err = float(np.abs(rgb - want[:, None, None, None]).max())
    print(f"grey axis {colour}: max error {err:.3e} (table off the axis by {off_axis:.3e})")
    assert err <= 2e-6 + off_axis


# ---------------------------------------------------------------------------------------------------------------- against float64
@pytest.mark.parametrize("colour", yuv.COLOURS)
def test_i420_to_rgb_against_float64(colour):
    rng = np.random.RandomState(11)
    for h, w in SIZES + [(16, 48)]:
        fr = rng.randint(0, 256, size=(3, yuv.i420_bytes(h, w)), dtype=np.uint8)          # limited-range legality is not assumed
        got = yuv.i420_to_rgb(fr, h, w, colour=colour)
        assert got.dtype == np.float32 and got.shape == (3, 3, h, w)
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
        err = float(np.abs(got.astype(np.float64) - _to_rgb64(fr, h, w, colour)).max())
        assert err <= 2e-6, (colour, h, w, err)


@pytest.mark.parametrize("colour", yuv.COLOURS)
def test_rgb_to_i420_against_float64(colour):
    rng = np.random.RandomState(5)
    pairs = []
    for H, W in SIZES + [(32, 40)]:
        x = rng.uniform(0.0, 1.0, size=(4, 3, H, W)).astype(np.float32)
        pairs.append((yuv.rgb_to_i420(x, colour=colour), _to_i420_64(x.astype(np.float64), colour)))
    _assert_rounds_to(pairs, colour)
    x = rng.uniform(-0.2, 1.2, size=(2, 3, 9, 11)).astype(np.float32)                      # the clamp; a NaN becomes 0
    x[0, 1, 3, 4] = np.nan
    x64 = np.nan_to_num(x.astype(np.float64), nan=0.0)
    _assert_rounds_to([(yuv.rgb_to_i420(x, colour=colour), _to_i420_64(x64, colour))], colour)


def _block_constant(n, h, w, seed):
    ch, cw = yuv.chroma_hw(h, w)
    x = np.random.RandomState(seed).uniform(0.05, 0.95, size=(n, 3, ch, cw)).astype(np.float32)          # no clamp is hit
    return np.repeat(np.repeat(x, 2, 2), 2, 3)[:, :, :h, :w].copy()


@pytest.mark.parametrize("colour", yuv.COLOURS)
@pytest.mark.parametrize("h,w", SIZES)
def test_round_trip_is_exact(colour, h, w):
    f = yuv.rgb_to_i420(_block_constant(6, h, w, seed=h * 31 + w), colour=colour)
    assert np.array_equal(yuv.rgb_to_i420(yuv.i420_to_rgb(f, h, w, colour=colour), colour=colour), f)


def test_bt601_to_bt709_conversion():
    pairs = []
    for h, w in SIZES + [(32, 40)]:
        f = yuv.rgb_to_i420(_block_constant(6, h, w, seed=w), colour="bt601")
        g = yuv.rgb_to_i420(yuv.i420_to_rgb(f, h, w, colour="bt601"), colour="bt709")
        assert g.shape == f.shape and not np.array_equal(g, f)
        pairs.append((g, _to_i420_64(_to_rgb64(f, h, w, "bt601"), "bt709")))
    _assert_rounds_to(pairs, "bt709")


def test_the_default_is_bt601_to_the_bit():
    rng = np.random.RandomState(2)
    for h, w in SIZES:
        fr = rng.randint(0, 256, size=(3, yuv.i420_bytes(h, w)), dtype=np.uint8)
        assert np.array_equal(yuv.i420_to_rgb(fr, h, w).view(np.uint32), yuv.i420_to_rgb(fr, h, w, colour="bt601").view(np.uint32))
        x = rng.uniform(-0.2, 1.2, size=(3, 3, h, w)).astype(np.float32)
        assert np.array_equal(yuv.rgb_to_i420(x), yuv.rgb_to_i420(x, colour="bt601"))
        for a, b in zip(yuv.ycbcr_f32(x), yuv.ycbcr_f32(x, colour="bt601")):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    t0, t1 = yuv.to_rgb_tables(), yuv.to_rgb_tables(yuv.matrix("bt601"))
    assert all(np.array_equal(t0[k], t1[k]) for k in t0)


# ------------------------------------------------------------------------------------------------- the public interface, on the host
def _net():
    from savsr_amd.archs.savsr_arch import SAVSR
    return SAVSR().eval()


def _i420(n, h=8, w=10):
    return torch.zeros(n, yuv.i420_bytes(h, w), dtype=torch.uint8)


RGB8 = torch.zeros(9, 8, 10, 3, dtype=torch.uint8)


@pytest.mark.parametrize("kwargs,frames,match", [
    (dict(pixel_format="i420", size=(8, 10), colour="bt2020"), _i420(9), "colour = 'bt2020': one of bt601, bt709, bt601-full, bt709-full"),
    (dict(pixel_format="i420", size=(8, 10), out="i420", out_colour="rec709"), _i420(9),
     "out_colour = 'rec709': one of bt601, bt709, bt601-full, bt709-full"),
    (dict(pixel_format="i420", size=(8, 10), colour=1), _i420(9), "colour = 1: one of bt601"),
    (dict(colour="bt709"), RGB8, "colour = 'bt709' goes with pixel_format = 'i420'"),
    (dict(out="i420", colour="bt709-full"), RGB8, "colour = 'bt709-full' goes with pixel_format = 'i420'"),
    (dict(pixel_format="i420", size=(8, 10), out_colour="bt709"), _i420(9), "out_colour = 'bt709' goes with out = 'i420'"),
    (dict(out="uint8", out_colour="bt601"), RGB8, "out_colour = 'bt601' goes with out = 'i420'"),
])
def test_upscale_video_refuses_bad_colour_arguments_without_a_gpu(kwargs, frames, match):
    from savsr_amd import VideoUpscaler
    with pytest.raises(ValueError, match=match):
        _net().upscale_video(frames, **kwargs)
    with pytest.raises(ValueError, match=match):
        VideoUpscaler(_net(), 4, **kwargs)


def test_good_colour_arguments_pass_every_host_check():
    from savsr_amd import VideoUpscaler
    for kw in (dict(pixel_format="i420", size=(8, 10), out="i420", colour="bt709"),
               dict(pixel_format="i420", size=(8, 10), out="i420", colour="bt601", out_colour="bt709"),
               dict(pixel_format="i420", size=(8, 10), colour="bt601-full"),
               dict(out="i420", out_colour="bt709")):
        frames = _i420(9) if "size" in kw else RGB8
        with pytest.raises(RuntimeError, match="AMD GPU only"):          # only the device is missing
            _net().upscale_video(frames, **kw)
        VideoUpscaler(_net(), 4, **kw)


# -------------------------------------------------------------------------------------------------------------------------- Y4M
def test_y4m_reader_colour_range():
    body = b"FRAME\n" + bytes(6)
    for tags, want in ((b" XCOLORRANGE=FULL", "full"), (b" XCOLORRANGE=LIMITED", "limited"), (b"", None), (b" XYSCSS=420JPEG", None),
                       (b" XYSCSS=420JPEG XCOLORRANGE=FULL", "full")):
        r = y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W2 H2 F25:1 Ip A1:1 C420jpeg" + tags + b"\n" + body))
        assert r.colour_range == want, tags
        assert [c.shape for c in r.chunks(4)] == [(1, 6)]


def test_y4m_writer_colour_range():
    f = io.BytesIO()
    w = y4m.Y4MWriter(f, 4, 2, (30, 1), "p", (1, 1))
    assert w.header == f.getvalue() == b"YUV4MPEG2 W4 H2 F30:1 Ip A1:1 C420jpeg\n"          # the default header, byte for byte
    for rng in ("full", "limited"):
        f = io.BytesIO()
        w = y4m.Y4MWriter(f, 4, 2, (30, 1), "p", (1, 1), colour_range=rng)
        assert f.getvalue() == b"YUV4MPEG2 W4 H2 F30:1 Ip A1:1 C420jpeg XCOLORRANGE=" + rng.upper().encode() + b"\n"
        frames = np.arange(2 * 12, dtype=np.uint8).reshape(2, 12)
        w.write(frames)
        f.seek(0)
        r = y4m.Y4MReader(f)
        assert r.colour_range == rng and (r.width, r.height, r.fps, r.aspect, r.colorspace) == (4, 2, (30, 1), (1, 1), "420jpeg")
        assert np.array_equal(np.concatenate(list(r.chunks(3))), frames)
    with pytest.raises(ValueError, match="colour_range = 'pc'"):
        y4m.Y4MWriter(io.BytesIO(), 4, 2, colour_range="pc")


# -------------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_colour_flags():
    from savsr_amd.upscale import parse_args
    base = ["--scale", "4", "--checkpoint", "x.pth"]
    a = parse_args(["-i", "in.y4m", "-o", "out.y4m"] + base)
    assert (a.colour, a.out_colour, a.colour_flags) == ("bt601", "same", False)
    a = parse_args(["-i", "in.y4m", "-o", "out.y4m", "--colour", "auto", "--out-colour", "bt709"] + base)
    assert (a.colour, a.out_colour, a.colour_flags) == ("auto", "bt709", True)
    a = parse_args(["-i", "in.y4m", "-o", "out.y4m", "--out-colour", "same"] + base)
    assert (a.colour, a.out_colour, a.colour_flags) == ("bt601", "same", True)
    for c in yuv.COLOURS:
        a = parse_args(["-i", "-", "-o", "-", "--colour", c, "--out-colour", c] + base)
        assert (a.colour, a.out_colour) == (c, c)
    assert parse_args(["-i", "lr", "-o", "out.y4m", "--out-colour", "auto"] + base).out_colour == "auto"
    assert parse_args(["-i", "in.y4m", "-o", "sr", "--colour", "bt709"] + base).colour == "bt709"
    for bad in (["-i", "in.y4m", "-o", "out.y4m", "--colour", "same"],            # `same` is the output's word
                ["-i", "in.y4m", "-o", "out.y4m", "--colour", "bt2020"],
                ["-i", "in.y4m", "-o", "out.y4m", "--out-colour", "rgb"],
                ["-i", "lr", "-o", "out.y4m", "--colour", "bt709"],               # PNG frames are RGB
                ["-i", "in.y4m", "-o", "sr", "--out-colour", "bt709"]):
        with pytest.raises(SystemExit):
            parse_args(bad + base)


def test_cli_auto_rule_and_resolution():
    from savsr_amd.upscale import auto_colour, resolve_colours
    assert auto_colour(576, 720, False) == "bt601"
    assert auto_colour(578, 720, False) == "bt709"
    assert auto_colour(360, 1280, False) == "bt709"
    assert auto_colour(180, 320, True) == "bt601-full" and auto_colour(720, 1280, True) == "bt709-full"
    lr, hr = (180, 320), (720, 1280)
    assert resolve_colours("bt601", "same", lr, hr, None) == ("bt601", "bt601")                 # the defaults
    assert resolve_colours("bt601", "same", lr, hr, "full") == ("bt601", "bt601")               # not auto: the tag is not followed
    assert resolve_colours("auto", "auto", lr, hr, None) == ("bt601", "bt709")                  # SD -> HD
    assert resolve_colours("auto", "auto", lr, hr, "limited") == ("bt601", "bt709")
    assert resolve_colours("auto", "auto", lr, hr, "full") == ("bt601-full", "bt709-full")      # the range from the tag, on both sides
    assert resolve_colours("auto", "same", hr, hr, "full") == ("bt709-full", "bt709-full")
    assert resolve_colours("auto", "bt709", (8, 10), (16, 20), "full") == ("bt601-full", "bt709")
    assert resolve_colours("bt709-full", "auto", lr, (360, 640), None) == ("bt709-full", "bt601-full")
    assert resolve_colours("bt601", "auto", None, hr, None) == (None, "bt709")                  # PNG folder in: limited range
    assert resolve_colours("bt601", "same", None, hr, None) == (None, "bt601")
    assert resolve_colours("auto", "same", lr, None, "full") == ("bt601-full", None)            # PNG folder out
