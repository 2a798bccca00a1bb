"""Ordered dither, the specification (savsr_amd/dither.py and dither= of yuv.rgb_to_i420 / yuv.unit_to_luma): the matrix, the three
properties that follow from the rule, what it is for (a ramp keeps its block means), the defaults, and the refusals.  No GPU."""
import numpy as np
import pytest

from savsr_amd import dither as D
from savsr_amd import scenes, yuv
from tests import dither_cases as DC


# ------------------------------------------------------------------------------------------------------------------------ 1. the matrix
def test_bayer_is_a_permutation_obeys_the_recursion_and_the_closed_form():
    B = D.bayer(16)
    assert B.shape == (16, 16) and sorted(B.ravel().tolist()) == list(range(256))
    b2 = np.array([[0, 2], [3, 1]])
    assert np.array_equal(D.bayer(2), b2)
    for n in (2, 4, 8):
        Bn, B2n = D.bayer(n), D.bayer(2 * n)
        y, x = np.mgrid[0:2 * n, 0:2 * n]
        assert np.array_equal(B2n, 4 * Bn[y % n, x % n] + b2[y // n, x // n])
    y, x = np.mgrid[0:16, 0:16]
    closed = sum(4 ** (3 - b) * (2 * (((x ^ y) >> b) & 1) + ((y >> b) & 1)) for b in range(4))
    assert np.array_equal(B, closed)
    assert B[0, :4].tolist() == [0, 128, 32, 160] and B[1, :4].tolist() == [192, 64, 224, 96]


def test_thresholds_are_exact_float32_inside_the_unit_interval():
    th = D.thresholds()
    assert th.dtype == np.float32 and th.shape == (16, 16)
    assert float(th.min()) > 0.0 and float(th.max()) < 1.0
    assert np.array_equal(th.astype(np.float64), (D.bayer(16).astype(np.float64) + 0.5) / 256.0)
    assert np.array_equal(D.threshold_field(20, 35), th[np.ix_(np.arange(20) % 16, np.arange(35) % 16)])
    assert D.dither_id(None) == 0 and D.dither_id("ordered") == 1 and D.DITHERS == ("ordered",)


# ----------------------------------------------------------------------------------------------------------------- 2. constant fields
def test_constant_fields_sum_exactly_and_integers_pass_unchanged():
    j = np.arange(256, dtype=np.float32) / np.float32(256)
    for i in DC.CONSTANT_I:
        t = (np.float32(i) + j)[:, None, None] * np.ones((1, 16, 16), np.float32)          # [256, 16, 16]: field j is i + j / 256
        assert np.array_equal(t[:, 0, 0].astype(np.float64), i + np.arange(256) / 256.0)  # (exact in float32)
        q = D.dither_floor(t)
        assert q.dtype == np.float32
        assert np.array_equal(q.reshape(256, -1).sum(1, dtype=np.float64), 256.0 * i + np.arange(256)), i
        assert float(np.abs(q - np.float32(i)).max()) <= 1.0
    for code in DC.EXACT_CODES:
        t = np.full((16, 16), code, np.float32)
        assert np.array_equal(D.dither_floor(t), t), code
    # any constant: the block mean is within 1 / 512 of t
    for t0 in np.random.RandomState(0).uniform(0, 255, size=50).astype(np.float32):
        q = D.dither_floor(np.full((16, 16), t0, np.float32))
        assert abs(float(q.mean(dtype=np.float64)) - float(t0)) <= 1.0 / 512 + 1e-12, t0


# --------------------------------------------------------------------------------------------------------------------------- 3. range
@pytest.mark.parametrize("chroma", yuv.CHROMAS)
def test_limited_range_stays_in_its_nominal_range_without_a_clip(chroma):
    x = DC.corners(16, 32)
    for colour in ("bt601", "bt709"):
        for depth in DC.DEPTHS:
            k = 1 << (depth - 8)
            y, u, v = yuv.split_planes(yuv.rgb_to_i420(x, colour, depth, chroma, dither="ordered"), 16, 32, depth, chroma)
            assert 16 * k <= int(y.min()) and int(y.max()) <= 235 * k, (colour, depth)
            for p in (u, v):
                assert 16 * k <= int(p.min()) and int(p.max()) <= 240 * k, (colour, depth)
            # (no clip hides an excursion: the unclipped rule's values are the ones written)
            for t, p in zip(yuv.ycbcr_f32(x, colour, chroma), (y, u, v)):
                assert np.array_equal(D.dither_floor(t * np.float32(k)), p.astype(np.float32))
    for colour in ("bt601-full", "bt709-full"):
        planes = yuv.split_planes(yuv.rgb_to_i420(x, colour, 8, chroma, dither="ordered"), 16, 32, 8, chroma)
        for t, p in zip(yuv.ycbcr_f32(x, colour, chroma), planes):
            assert np.array_equal(np.clip(D.dither_floor(t), 0, 255), p.astype(np.float32))          # 0 .. 255: the clip that follows rint


# ------------------------------------------------------------------------------------------------------------------ 4. the point of it
def test_a_two_code_ramp_keeps_its_block_means_with_the_dither_and_bands_without():
    x = DC.ramp()
    t = np.fmin(np.fmax(x, np.float32(0)), np.float32(1)) * np.float32(255)
    cases = [("rgb_to_u8", DC.block_means(t[0]), lambda d: D.rgb_to_u8(x, dither=d)[0].transpose(2, 0, 1))]
    for colour in yuv.COLOURS:
        ty = yuv.ycbcr_f32(x, colour)[0]
        cases.append((colour, DC.block_means(ty[0]), lambda d, c=colour: yuv.split_planes(yuv.rgb_to_i420(x, c, 8, dither=d), 32, 512)[0][0]))
    for name, want, make in cases:
        err_d = float(np.abs(DC.block_means(make("ordered")) - want).max())
        err_n = float(np.abs(DC.block_means(make(None)) - want).max())
        print(f"{name}: largest block-mean error {err_d:.4f} code dithered, {err_n:.4f} rounded")
        assert err_d <= 1.0 / 64, (name, err_d)
        assert err_n >= 1.0 / 4, (name, err_n)


# ------------------------------------------------------------------------------------------------------------------------ 5. defaults
def test_dither_none_is_the_existing_rounding():
    for H, W in ((6, 16), (5, 3), (30, 35)):
        x = DC.float_in(2, 3, H, W)
        for chroma in yuv.CHROMAS:
            for depth in DC.DEPTHS:
                for colour in (yuv.COLOURS if depth == 8 else yuv.COLOURS[:2]):
                    for siting in DC.sitings(chroma):
                        k = np.float32(1 << (depth - 8))
                        planes = [np.rint(v * k) for v in yuv.ycbcr_f32(x, colour, chroma, siting)]
                        if yuv.is_full_range(colour):
                            planes = [np.clip(v, 0, 255) for v in planes]
                        want = np.concatenate([v.astype(np.uint8 if depth == 8 else "<u2").reshape(2, -1) for v in planes], 1).view(np.uint8)
                        assert np.array_equal(yuv.rgb_to_i420(x, colour, depth, chroma, siting, dither=None), want)
                        assert np.array_equal(yuv.rgb_to_i420(x, colour, depth, chroma, siting), want)
        for depth in DC.DEPTHS:
            want = np.rint(np.fmin(np.fmax(x, np.float32(0)), np.float32(1)) * np.float32(255 << (depth - 8)))
            for got in (yuv.unit_to_luma(x, depth, dither=None), yuv.unit_to_luma(x, depth)):
                assert got.dtype == (np.uint8 if depth == 8 else np.uint16) and np.array_equal(got, want)
        for c in (1, 3):
            xc = DC.float_in(2, c, H, W)
            want = scenes.quantize_u8(xc).transpose(0, 2, 3, 1)
            assert np.array_equal(D.rgb_to_u8(xc, dither=None), want) and np.array_equal(D.rgb_to_u8(xc), want)
            assert not np.array_equal(D.rgb_to_u8(xc, dither="ordered"), want)


def test_the_dithered_conversions_are_the_rule_per_plane():
    x = DC.float_in(2, 3, 30, 35)
    got = yuv.rgb_to_i420(x, "bt709", 10, "420", "left", dither="ordered")
    planes = [D.dither_floor(v * np.float32(4)) for v in yuv.ycbcr_f32(x, "bt709", "420", "left")]
    assert np.array_equal(got, np.concatenate([v.astype("<u2").reshape(2, -1) for v in planes], 1).view(np.uint8))
    t = np.fmin(np.fmax(x, np.float32(0)), np.float32(1)) * np.float32(255 * 16)
    assert np.array_equal(yuv.unit_to_luma(x, 12, dither="ordered"), D.dither_floor(t).astype(np.uint16))
    # one threshold per pixel, shared by its channels: equal channels stay equal
    g = np.repeat(DC.float_in(1, 1, 17, 33), 3, axis=1)
    u8 = D.rgb_to_u8(g, dither="ordered")
    assert np.array_equal(u8[..., 0], u8[..., 1]) and np.array_equal(u8[..., 0], u8[..., 2])


# ----------------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_by_name():
    from savsr_amd.video import video_spec
    from savsr_amd.upscale import parse_args
    x = np.zeros((1, 3, 4, 4), np.float32)
    for call in (lambda d: D.check_dither(d), lambda d: D.rgb_to_u8(x, dither=d), lambda d: yuv.rgb_to_i420(x, dither=d),
                 lambda d: yuv.unit_to_luma(x, dither=d), lambda d: video_spec(3, out="uint8", dither=d)):
        with pytest.raises(ValueError, match="dither = 'bayer': None or one of ordered"):
            call("bayer")
        for bad in (1, True, ("ordered",)):
            with pytest.raises(ValueError, match="None or one of ordered"):
                call(bad)
    with pytest.raises(ValueError, match="dither = 'ordered' goes with an integer output .*out = 'float' has nothing to quantise"):
        video_spec(3, dither="ordered")
    with pytest.raises(ValueError, match="out = 'float' has nothing to quantise"):
        video_spec(3, out="float", pixel_format="i420", size=(4, 4), dither="ordered")
    assert video_spec(3, out="uint8", dither="ordered").dither == "ordered" and video_spec(3, out="i420").dither is None
    common = ["-i", "a", "-o", "b", "--scale", "2", "--checkpoint", "c"]
    with pytest.raises(SystemExit):
        parse_args(common + ["--dither", "bogus"])
    assert parse_args(common).dither is None and parse_args(common + ["--dither", "none"]).dither is None
    assert parse_args(common + ["--dither", "ordered"]).dither == "ordered"
