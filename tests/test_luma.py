"""Luma-only checkpoints on YUV and grey-scale video, the host side: the numpy specification of luma.hip (savsr_amd/yuv.py: luma_to_unit,
unit_to_luma, chroma_axis_table, resample_chroma), the argument checks of chroma_filter= / "y400", and Cmono in the Y4M reader and writer."""
import io

import numpy as np
import pytest
import torch

from savsr_amd import yuv
from savsr_amd.packing import get_hw
from tests.channel_cases import CHANNEL_CASES

LAYOUTS = yuv.CHROMAS
SITINGS = (None,) + yuv.SITINGS


def _valid(siting, chroma):
    return not (siting == "topleft" and chroma == "422")


# ---------------------------------------------------------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("depth", yuv.DEPTHS)
@pytest.mark.parametrize("chroma", LAYOUTS)
@pytest.mark.parametrize("h,w", [(5, 3), (6, 8), (7, 6)])
def test_identity_returns_the_plane(h, w, chroma, depth):
    ch, cw = yuv.chroma_hw(h, w, chroma)
    plane = np.random.RandomState(h + w + depth).randint(0, 1 << depth, size=(2, ch, cw)).astype(np.uint8 if depth == 8 else np.uint16)
    for siting in SITINGS:
        if not _valid(siting, chroma):
            continue
        ty, tx = yuv.chroma_tables(h, w, h, w, chroma, chroma, siting, siting)
        for t in (ty, tx):
            assert t[2].shape[1] == 1 and (t[1] == 1).all() and (t[2] == 1.0).all() and t[0].tolist() == list(range(len(t[0])))
        out = yuv.resample_chroma(plane, ty, tx, depth, depth)
        assert out.dtype == plane.dtype and np.array_equal(out, plane)


# ---------------------------------------------------------------------------------------------------------------- 2. constant plane
@pytest.mark.parametrize("case", CHANNEL_CASES, ids=[c[0] for c in CHANNEL_CASES])
def test_a_constant_plane_stays_constant(case):
    _, _, h, w, scale = case
    H, W = get_hw(h, w, scale)
    for chroma in LAYOUTS:
        for out_chroma in LAYOUTS:
            for siting, out_siting in ((None, None), ("left", "left"), ("centre", "topleft"), ("topleft", "centre")):
                if not (_valid(siting, chroma) and _valid(out_siting, out_chroma)):
                    continue
                ty, tx = yuv.chroma_tables(h, w, H, W, chroma, out_chroma, siting, out_siting)
                for d, D, v in ((8, 8, 77), (8, 10, 255), (10, 8, 513), (12, 12, 4095), (8, 8, 0)):
                    plane = np.full(yuv.chroma_hw(h, w, chroma), v, np.uint16)
                    out = yuv.resample_chroma(plane, ty, tx, d, D)
                    want = int(np.rint(np.float32(v) * np.float32(2.0 ** (D - d))))          # (513 / 4 = 128.25 -> 128)
                    assert out.shape == yuv.chroma_hw(H, W, out_chroma) and (out == want).all(), (chroma, out_chroma, siting, out_siting, d, D)


# ---------------------------------------------------------------------------------------------------------------- 3. positions
def _positions(n_luma, sub, siting, axis):
    o = 0.0 if (siting == "topleft" or (siting == "left" and axis == "x")) else (sub - 1) / 2.0
    return sub * np.arange(-(-n_luma // sub)) + o


@pytest.mark.parametrize("scale", [(1.5, 1.5), (2, 2), (2.7, 3.3)])
def test_a_ramp_comes_out_at_the_output_sitings_positions(scale):
    """A linear ramp in luma coordinates sampled at siting_in's positions comes out as the same ramp at siting_out's positions, within 1 code
    >= 3 samples from the border, of the output plane and -- the border fold bends a ramp -- of the input plane too; at 48 x 50 luma that
    leaves at least 16 checked samples per axis.  10-bit codes and a slope of 8 codes per LR luma pixel: a wrong siting (half a chroma sample, sub / 2
    luma pixels) misses by 8 * sub / 2 >= 4 codes wherever the siting matters (sub = 2)."""
    h, w = 48, 50
    H, W = get_hw(h, w, scale)
    slope, base, d = 8.0, 100.0, 10
    worst = 0.0
    for chroma in LAYOUTS:
        for out_chroma in LAYOUTS:
            (sy, sx), (oy, ox) = yuv.subsampling(chroma), yuv.subsampling(out_chroma)
            for siting in SITINGS:
                for out_siting in SITINGS:
                    if not (_valid(siting, chroma) and _valid(out_siting, out_chroma)):
                        continue
                    ty, tx = yuv.chroma_tables(h, w, H, W, chroma, out_chroma, siting, out_siting)
                    for table, n_in, n_out, s_in, s_out, axis in ((tx, w, W, sx, ox, "x"), (ty, h, H, sy, oy, "y")):
                        pin = _positions(n_in, s_in, siting, axis)
                        line = np.rint(base + slope * pin).astype(np.uint16)
                        plane = np.repeat(line[None, :], 7, 0) if axis == "x" else np.repeat(line[:, None], 7, 1)
                        one = (np.arange(7, dtype=np.int32), np.ones(7, np.int32), np.ones((7, 1), np.float32))          # identity on the other axis
                        out = yuv.resample_chroma(plane, one if axis == "x" else table, table if axis == "x" else one, d, d)
                        got = (out[3] if axis == "x" else out[:, 3]).astype(np.float64)
                        pout = _positions(n_out, s_out, out_siting, axis)
                        want = base + slope * ((pout + 0.5) * n_in / n_out - 0.5)
                        # the source must be interior too: >= 3 input samples from the border
                        u = ((pout + 0.5) * n_in / n_out - 0.5 - (pin[0])) / s_in
                        ok = (u >= 3) & (u <= len(pin) - 4)
                        ok[:3] = False
                        ok[len(ok) - 3:] = False
                        assert ok.sum() >= 16, (chroma, out_chroma, axis, scale, int(ok.sum()))
                        err = np.abs(got - want)[ok].max()
                        worst = max(worst, err)
                        assert err <= 1.0, (chroma, out_chroma, siting, out_siting, axis, err)
    print(f"ramp at x{scale}: worst interior error {worst:.3f} codes")


def test_a_wrong_siting_would_miss_by_four_codes():
    """The sensitivity of the test above: reading left-sited 4:2:0 samples as centre-sited shifts the result by slope * sub / 2 = 8 codes."""
    h, w, H, W = 24, 26, 48, 52
    pin = _positions(w, 2, "left", "x")
    plane = np.repeat(np.rint(100 + 8.0 * pin).astype(np.uint16)[None, :], 5, 0)
    one = (np.arange(5, dtype=np.int32), np.ones(5, np.int32), np.ones((5, 1), np.float32))
    right = yuv.resample_chroma(plane, one, yuv.chroma_axis_table(w, W, 2, 2, "left", "left", "x"), 10, 10)[2].astype(int)
    wrong = yuv.resample_chroma(plane, one, yuv.chroma_axis_table(w, W, 2, 2, "centre", "left", "x"), 10, 10)[2].astype(int)
    assert np.abs(right - wrong)[4:-4].min() >= 4


# ---------------------------------------------------------------------------------------------------------------- 4. the reference's bicubic
@pytest.mark.parametrize("cw,cW", [(8, 20), (12, 30), (32, 24), (64, 16)])
def test_axis_table_is_the_core_bicubic(cw, cW):
    """Centre / None siting on both sides, the same layout, even sizes with cW / cw = W / w: the dense [out][in] matrix is that of
    resize_gpu.core_tables (pinned to core.py by tests/golden/core_resize.npz).  core_tables evaluates positions in float32, so a few ulp
    of the position (<= 64) times the kernel's largest slope (1.39), on the weight and on its normaliser: 4 * 2^-24 * 64 * 1.39 * 2."""
    from savsr_amd.resize_gpu import core_tables
    ref = yuv.dense_axis(core_tables(cw, cW), cw)
    worst = 0.0
    for sub in (1, 2):
        for si, so in ((None, None), ("centre", "centre"), (None, "centre")):
            got = yuv.dense_axis(yuv.chroma_axis_table(cw * sub, cW * sub, sub, sub, si, so, "x"), cw)
            worst = max(worst, float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()))
    print(f"chroma_axis_table vs core_tables {cw} -> {cW}: worst difference {worst:.3e}")
    assert worst <= 4 * 2.0 ** -24 * 64 * 1.39 * 2


def test_axis_table_shape_and_normalisation():
    for args in ((13, 35, 2, 2, "left", "centre", "x"), (17, 56, 2, 1, None, None, "y"), (20, 30, 1, 2, "topleft", "topleft", "y"), (3, 7, 2, 2, "left", "left", "x")):
        xmin, xsize, wt = yuv.chroma_axis_table(*args)
        n_in, n_out = -(-args[0] // args[2]), -(-args[1] // args[3])
        assert xmin.dtype == np.int32 and xsize.dtype == np.int32 and wt.dtype == np.float32 and len(xmin) == len(xsize) == len(wt) == n_out
        assert (xmin >= 0).all() and (xmin + xsize <= n_in).all() and (xsize >= 1).all() and wt.shape[1] == xsize.max()
        assert np.allclose(wt.sum(1), 1.0, atol=1e-6)
        for j in range(n_out):
            assert (wt[j, xsize[j]:] == 0).all()
    with pytest.raises(ValueError, match="sub_in, sub_out = 3, 2"):
        yuv.chroma_axis_table(8, 16, 3, 2)
    with pytest.raises(ValueError, match="siting = 'middle'"):
        yuv.chroma_axis_table(8, 16, 2, 2, "middle")


def test_downscaling_stretches_the_kernel():
    """4:4:4 in, 4:2:0 out at x 1.5: rho = 2 / 1.5 input samples per output sample, ceil(4 rho) + 2 = 8 taps before folding and trimming."""
    xmin, xsize, wt = yuv.chroma_axis_table(40, 60, 1, 2, None, None, "x")
    assert 6 <= wt.shape[1] <= 8 and len(xmin) == 30


# ---------------------------------------------------------------------------------------------------------------- 5. roundings
@pytest.mark.parametrize("depth", yuv.DEPTHS)
def test_luma_round_trip_is_exact(depth):
    """unit_to_luma(luma_to_unit(s)) == s for every code the output rule can give, 0 .. 255 k: every code at 8 bits.  At 10 / 12 bits the two
    rules as specified cannot return the codes above 255 k (1021 .. 1023, 4081 .. 4095: luma_to_unit puts them above 1.0, and unit_to_luma
    clamps to 1.0 as savsr_video_quantize_u8 does); those reserved codes come back as 255 k, which is asserted here as well."""
    k = 1 << (depth - 8)
    s = np.arange(1 << depth)
    unit = yuv.luma_to_unit(s, depth)
    assert unit.dtype == np.float32 and unit[0] == 0 and unit[255 * k] == 1
    assert np.array_equal(yuv.unit_to_luma(unit, depth), np.minimum(s, 255 * k))
    top = np.float32((1 << depth) - 1) / np.float32(255 * k)
    assert yuv.luma_to_unit(np.array([1 << depth, 65535]), depth).tolist() == [top, top]           # above 2^d - 1: read as 2^d - 1
    assert yuv.unit_to_luma(np.array([np.nan, -1.0, 2.0, np.inf], np.float32), depth).tolist() == [0, 0, (255 << (depth - 8)), (255 << (depth - 8))]


def test_eight_bit_rules_are_the_u8_paths():
    from savsr_amd.scenes import quantize_u8
    s = np.arange(256, dtype=np.uint8)
    assert np.array_equal(yuv.luma_to_unit(s, 8), s.astype(np.float32) / np.float32(255.0))          # savsr_video_gather_u8's table
    x = np.random.RandomState(0).uniform(-0.1, 1.1, 4096).astype(np.float32)
    x[:6] = [np.nan, 0.5 / 255, 1.5 / 255, 2.5 / 255, -0.0, 1.0]
    assert np.array_equal(yuv.unit_to_luma(x, 8), quantize_u8(x))                                   # savsr_video_quantize_u8's rule
    assert yuv.unit_to_luma(np.float32([0.5 / 255, 1.5 / 255, 2.5 / 255]), 8).tolist() == [0, 2, 2]  # half to even


def test_resample_overshoot_is_clipped_and_depths_convert():
    ty, tx = yuv.chroma_tables(8, 8, 16, 16, "444", "444")
    plane = np.zeros((8, 8), np.uint8)
    plane[:, 4:] = 255
    out = yuv.resample_chroma(plane, ty, tx)
    assert out.min() == 0 and out.max() == 255
    wide = yuv.resample_chroma(plane, ty, tx, 8, 10)
    assert wide.dtype == np.uint16 and wide.max() == 1023 and wide[0, -1] == 1020 and yuv.resample_chroma(wide * 0 + 4095, *yuv.chroma_tables(16, 16, 16, 16, "444", "444"), 12, 8).max() == 255
    over = yuv.resample_chroma(np.full((8, 8), 60000, np.uint16), ty, tx, 10, 10)
    assert (over == 1023).all()                                                                      # samples above 2^d - 1 are clipped first


def test_luma_only_frames_assembles_the_planes():
    h, w, H, W = 6, 8, 12, 20
    frames = np.random.RandomState(1).randint(0, 256, size=(3, yuv.frame_bytes(h, w))).astype(np.uint8)
    sr = np.random.RandomState(2).uniform(0, 1, size=(3, 1, H, W)).astype(np.float32)
    out = yuv.luma_only_frames(frames, h, w, sr, out_chroma="444", siting="left")
    y, u, v = yuv.split_planes(out, H, W, 8, "444")
    ty, tx = yuv.chroma_tables(h, w, H, W, "420", "444", "left", None)
    _, u0, v0 = yuv.split_planes(frames, h, w)
    assert np.array_equal(y, yuv.unit_to_luma(sr[:, 0])) and np.array_equal(u, yuv.resample_chroma(u0, ty, tx)) and np.array_equal(v, yuv.resample_chroma(v0, ty, tx))
    mono = yuv.luma_only_frames(frames, h, w, sr, out_depth=10, out_chroma=yuv.MONO)
    assert mono.shape == (3, yuv.frame_bytes(H, W, 10, yuv.MONO)) == (3, 2 * H * W)
    with pytest.raises(ValueError, match="grey-scale frames have no chroma planes"):
        yuv.luma_only_frames(frames[:, :h * w], h, w, sr, chroma=yuv.MONO, out_chroma="420")


# ---------------------------------------------------------------------------------------------------------------- 6. defaults and refusals
def _net(nch):
    from savsr_amd.archs.savsr_arch import SAVSR
    return SAVSR(num_in_ch=nch, num_feat=32).eval()


@pytest.fixture(scope="module")
def net1():
    return _net(1)


def _i420(n=9, h=8, w=10, depth=8, chroma="420"):
    return torch.zeros(n, yuv.frame_bytes(h, w, depth, chroma), dtype=torch.uint8)


def _refused(net, match, frames=None, **kw):
    from savsr_amd import VideoUpscaler
    kw.setdefault("pixel_format", "i420")
    kw.setdefault("size", (8, 10))
    with pytest.raises(ValueError, match=match):
        net.upscale_video(_i420() if frames is None else frames, 2, **kw)
    with pytest.raises(ValueError, match=match):
        VideoUpscaler(net, 2, **kw).push(_i420() if frames is None else frames)


def test_without_chroma_filter_the_two_refusals_are_unchanged(net1):
    _refused(net1, "I420 frames are colour frames, the network takes num_in_ch = 1")
    _refused(net1, "out = 'i420' holds colour frames", out="i420")
    _refused(net1, "I444 frames are colour frames, the network takes num_in_ch = 1", pixel_format="i444", frames=_i420(chroma="444"))


def test_luma_path_refusals_by_name(net1):
    _refused(net1, "chroma_filter = 'lanczos': None or one of bicubic", chroma_filter="lanczos")
    _refused(_net(3), "chroma_filter = 'bicubic' with num_in_ch = 3: chroma goes through such a network", chroma_filter="bicubic")
    _refused(net1, "colour = 'bt601', out_colour = 'bt709': a luma-only network never forms RGB", out="i420", out_colour="bt709",
             chroma_filter="bicubic")
    _refused(net1, "siting = 'topleft' with 4:2:2 chroma", pixel_format="i422", siting="topleft", chroma_filter="bicubic", frames=_i420(chroma="422"))
    _refused(net1, "out_siting = 'topleft' with 4:2:2 chroma", out="i422", out_siting="topleft", chroma_filter="bicubic")
    _refused(net1, "pixel_format = 'y400' frames have no chroma planes: out = 'i420' cannot be made from them", pixel_format="y400", out="i420",
             chroma_filter="bicubic", frames=torch.zeros(9, 80, dtype=torch.uint8))
    _refused(_net(3), "pixel_format = 'y400' holds grey-scale frames, the network takes num_in_ch = 3", pixel_format="y400",
             frames=torch.zeros(9, 80, dtype=torch.uint8))
    _refused(_net(3), "out = 'y400' holds grey-scale frames, the network takes num_in_ch = 3", out="y400", pixel_format="rgb", size=None,
             frames=torch.zeros(9, 8, 10, 3, dtype=torch.uint8))
    _refused(net1, "out = 'i420' from a luma-only network goes with pixel_format = 'i420', 'i422' or 'i444' or 'y400'", out="i420", pixel_format="rgb",
             size=None, chroma_filter="bicubic", frames=torch.zeros(9, 8, 10, 1, dtype=torch.uint8))
    _refused(net1, "chroma_filter = 'bicubic' goes with pixel_format = 'i420', 'i422' or 'i444': 'rgb' frames have no chroma planes", pixel_format="rgb",
             size=None, chroma_filter="bicubic", frames=torch.zeros(9, 8, 10, 1, dtype=torch.uint8))
    _refused(net1, "Y400 frames of 8 x 10 have 80 bytes, got 120", pixel_format="y400")
    _refused(net1, r"10-bit I420 frames of 8 x 10 have 240 bytes \(16-bit samples\), got 120", depth=10, chroma_filter="bicubic")


def test_accepted_calls_stop_at_the_missing_device_only(net1):
    """The network stays on the host, so every accepted call ends at the device check, with or without a GPU in the machine."""
    for kw in (dict(chroma_filter="bicubic"), dict(chroma_filter="bicubic", out="i444", out_depth=10, siting="left", out_siting=None),
               dict(chroma_filter="bicubic", out="y400"), dict(out="y400")):
        with pytest.raises(RuntimeError, match="AMD GPU only"):
            net1.upscale_video(_i420(), 2, pixel_format="i420", size=(8, 10), **kw)
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        net1.upscale_video(torch.zeros(9, 160, dtype=torch.uint8), 2, pixel_format="y400", size=(8, 10), depth=10, out="y400")


def test_frame_bytes_of_grey_scale_frames():
    assert yuv.frame_bytes(5, 7, 8, "400") == 35 and yuv.frame_bytes(5, 7, 12, yuv.MONO) == 70 and yuv.layout_name("400") == "Y400"
    assert yuv.frame_bytes(5, 7) == 35 + 2 * 12


def test_pair_sad_spec_reads_grey_scale_frames():
    from savsr_amd.scenes import pair_sad, sad_samples
    y = np.random.RandomState(0).randint(0, 256, size=(4, 6, 5)).astype(np.uint8)
    assert pair_sad(y.reshape(4, -1), "y400", (6, 5)).tolist() == pair_sad(y[..., None]).tolist()
    y12 = (y.astype("<u2") << 4).reshape(4, -1).view(np.uint8)
    assert pair_sad(y12, "y400", (6, 5), 12).tolist() == pair_sad(y[..., None]).tolist() and sad_samples((4, 30), "y400", (6, 5)) == 30


def test_cmono_header_round_trips_and_the_default_reader_refuses_it():
    from savsr_amd.y4m import Y4MReader, Y4MWriter
    for depth, tag in ((8, "mono"), (10, "mono10"), (12, "mono12")):
        buf = io.BytesIO()
        wr = Y4MWriter(buf, 7, 5, (30, 1), depth=depth, chroma="400")
        assert wr.frame_bytes == yuv.frame_bytes(5, 7, depth, "400") and f" C{tag}\n".encode() in wr.header
        frames = np.random.RandomState(depth).randint(0, 256, size=(3, wr.frame_bytes)).astype(np.uint8)
        wr.write(frames)
        buf.seek(0)
        rd = Y4MReader(buf, high_depth=True, mono=True)
        assert (rd.width, rd.height, rd.fps, rd.depth, rd.chroma, rd.colorspace, rd.siting) == (7, 5, (30, 1), depth, "400", tag, None)
        assert np.array_equal(np.concatenate(list(rd.chunks(2)), 0), frames)
        buf.seek(0)
        with pytest.raises(ValueError, match=f"colour space tag 'C{tag}' is not supported: 8-bit 4:2:0 only"):
            Y4MReader(buf)
        buf.seek(0)
        with pytest.raises(ValueError, match=f"colour space tag 'C{tag}' is not supported: 4:2:0, 4:2:2, 4:4:4 at 8, 10 or 12 bits only"):
            Y4MReader(buf, high_depth=True, layouts=yuv.CHROMAS)
    buf = io.BytesIO(b"YUV4MPEG2 W4 H4 Cmono10\n")
    with pytest.raises(ValueError, match="'Cmono10' is not supported"):
        Y4MReader(buf, mono=True)                    # high depth is its own opt-in


def test_cli_flag():
    from savsr_amd import upscale
    a = upscale.parse_args(["-i", "a.y4m", "-o", "b.y4m", "--scale", "2", "--checkpoint", "x.pth"])
    assert a.chroma_filter is None
    a = upscale.parse_args(["-i", "a.y4m", "-o", "b.y4m", "--scale", "2", "--checkpoint", "x.pth", "--chroma-filter", "bicubic"])
    assert a.chroma_filter == "bicubic"
    with pytest.raises(SystemExit):
        upscale.parse_args(["-i", "a", "-o", "b.y4m", "--scale", "2", "--checkpoint", "x.pth", "--chroma-filter", "bicubic"])
