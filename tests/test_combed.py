"""The specification of combed= (savsr_amd/pulldown.py `comb_windows`, `combed_from_windows`, `remove_pulldown_frames(combed=...)`) on
hand-computed matrices, the property that makes it safe on clean film (no recovered film frame is flagged, so combed= changes nothing
there), what it is for (a hybrid of telecined film and truly interlaced video: exactly the insert's frames are flagged and come out
clean), the refusals and the command line's flags.  No GPU needed."""
import numpy as np
import pytest
import torch

from savsr_amd import pulldown as pd
from savsr_amd.deinterlace import DEINTERLACERS, FIELD_ORDERS, deinterlace_frames
from tests import combed_cases as cc
from tests.pulldown_cases import KINDS, packed_film, planar_film


def _patch(r, c, y0, x0, order="tff", step=1, hi=255):
    """[1, r, c]: zeros with the second-field rows of the 16-row x 16-pixel patch at (y0, x0) set to `hi`: there a = c = 0, b = hi, the
    measure is 2 hi, and it is 0 on every other second-field sample."""
    q = 1 - pd.first_parity(order)
    m = np.zeros((1, r, c), np.int64)
    ys = [y for y in range(y0, min(y0 + 16, r)) if y % 2 == q]
    m[0][np.ix_(ys, range(x0, min(x0 + 16 * step, c)))] = hi
    return m


def _brute(m, order, step=1, threshold=9, depth=8):
    """comb_windows sample by sample and window by window."""
    p = pd.first_parity(order)
    v = np.minimum(np.asarray(m).astype(np.int64), (1 << depth) - 1) >> (depth - 8)
    n, r, c = v.shape
    out = np.zeros((n, 2), np.int64)
    for k in range(n):
        comb = np.zeros((r, c), np.int64)
        for y in range(1, r - 1):
            if y % 2 != p:
                a, b, e = v[k, y - 1], v[k, y], v[k, y + 1]
                comb[y] = np.abs(a - b) + np.abs(e - b) - np.abs(a - e) > 2 * threshold
        out[k, 1] = comb.sum()
        out[k, 0] = max(comb[y0:y0 + 16, x0:x0 + 16 * step].sum() for y0 in range(0, r, 8) for x0 in range(0, c, 8 * step))
    return out


# ---------------------------------------------------------------------------------------------------------------------- the measure
def test_a_fully_combed_patch_reads_its_second_field_samples():
    """16 x 16 holds 8 second-field rows of 16: 128 where a window lies on the patch; at (4, 4) the best windows cover 12 x 12 of it."""
    for (y0, x0), best in (((0, 0), 128), ((8, 8), 128), ((4, 4), 72)):
        assert pd.comb_windows(_patch(40, 40, y0, x0), "tff").tolist() == [[best, 128]], (y0, x0)
    # bff: the second field is the even rows; row 0 has no row above it, so a patch at the top has 7 scored rows
    assert pd.comb_windows(_patch(40, 40, 0, 0, "bff"), "bff").tolist() == [[7 * 16, 7 * 16]]
    assert pd.comb_windows(_patch(40, 40, 8, 16, "bff"), "bff").tolist() == [[128, 128]]
    # the windows overlap by half: a patch on no cell boundary is still seen whole by no window, and never read as less than a quarter
    assert pd.comb_windows(_patch(40, 40, 4, 8), "tff").tolist() == [[96, 128]]


def test_a_patch_on_the_last_rows_and_columns_of_an_odd_sized_matrix():
    """33 x 41: rows 17 .. 32, of which the second-field rows (tff: odd) with a row below are 17 .. 31; columns 25 .. 40.  The window at
    (16, 24) holds columns 24 .. 39, 15 of the patch's 16; the clipped window at (16, 32) holds its last 9."""
    m = _patch(33, 41, 17, 25)
    assert pd.comb_windows(m, "tff").tolist() == [[8 * 15, 8 * 16]]
    m = _patch(33, 41, 25, 33)                        # the last cell row and column alone: rows 25 .. 31 odd (4), columns 33 .. 40 (8)
    assert pd.comb_windows(m, "tff").tolist() == [[32, 32]]
    assert np.array_equal(pd.comb_windows(m, "tff"), _brute(m, "tff"))


def test_rows_2_3_4():
    rng = np.random.RandomState(0)
    for order in FIELD_ORDERS:
        assert not pd.comb_windows(rng.randint(0, 256, size=(2, 2, 20)), order).any()
        assert not pd.comb_windows(rng.randint(0, 256, size=(2, 1, 20)), order).any()
    three = np.zeros((1, 3, 20), np.int64)
    three[0, 1] = 255
    assert pd.comb_windows(three, "tff").tolist() == [[16, 20]]          # y = 1 is a second-field row of tff alone
    assert pd.comb_windows(three, "bff").tolist() == [[0, 0]]
    four = np.zeros((1, 4, 20), np.int64)
    four[0, 1:3] = 255                                                   # rows 1 (tff) and 2 (bff): each between a 0 and a 255 row: not combed
    assert pd.comb_windows(four, "tff").tolist() == [[0, 0]] and pd.comb_windows(four, "bff").tolist() == [[0, 0]]
    four[0, 2] = 0
    four[0, 3] = 0
    assert pd.comb_windows(four, "tff").tolist() == [[16, 20]] and pd.comb_windows(four, "bff").tolist() == [[0, 0]]
    four[0, 1], four[0, 2] = 0, 255
    assert pd.comb_windows(four, "tff").tolist() == [[0, 0]] and pd.comb_windows(four, "bff").tolist() == [[16, 20]]


def test_the_threshold_boundary():
    """a = c = 0: the measure is 2 b.  2 b = 2 T is not combed, 2 T + 1 cannot occur there; with a = 0, c = 1 and b = T + 1 it is 2 T + 1."""
    for t in (0, 9, 100, 254):
        m = np.zeros((1, 5, 4), np.int64)
        m[0, 1] = t                                   # 2 t = 2 T
        assert pd.comb_windows(m, "tff", threshold=t).tolist() == [[0, 0]]
        m[0, 2] = 1
        m[0, 1] = t + 1                               # |0 - b| + |1 - b| - 1 = 2 t + 1 - 1 + ... : (t + 1) + t - 1 = 2 t: still not combed
        assert pd.comb_windows(m, "tff", threshold=t).tolist() == [[0, 0]]
        m[0, 1] = t + 1
        m[0, 2] = 0                                   # 2 (t + 1) = 2 T + 2
        assert pd.comb_windows(m, "tff", threshold=t).tolist() == [[4, 4]]
    m = np.zeros((1, 3, 1), np.int64)
    m[0, :, 0] = (0, 10, 1)                           # 10 + 9 - 1 = 18 = 2 * 9: not combed
    assert pd.comb_windows(m, "tff").tolist() == [[0, 0]]
    m[0, :, 0] = (0, 11, 2)                           # 11 + 9 - 2 = 18
    assert pd.comb_windows(m, "tff").tolist() == [[0, 0]]
    m[0, :, 0] = (1, 11, 0)                           # 10 + 11 - 1 = 20 > 18; an odd measure: (0, 10, 1) above is 18, (0, 11, 1) is 20
    assert pd.comb_windows(m, "tff").tolist() == [[1, 1]]
    m[0, :, 0] = (3, 0, 40)                           # below the interval: 3 + 40 - 37 = 6
    assert pd.comb_windows(m, "tff", threshold=2).tolist() == [[1, 1]] and pd.comb_windows(m, "tff", threshold=3).tolist() == [[0, 0]]


def test_step_3_cells_are_8_pixels_of_3_samples():
    """A patch of 16 pixels x 3 samples at pixel 8: one window holds its 8 x 48 samples; with step 1 the same matrix is a patch 48 samples
    wide, of which a window holds 16 columns."""
    m = _patch(40, 120, 8, 24, step=3)
    assert pd.comb_windows(m, "tff", step=3).tolist() == [[8 * 48, 8 * 48]]
    assert pd.comb_windows(m, "tff", step=1).tolist() == [[128, 8 * 48]]
    assert pd.combed_from_windows(pd.comb_windows(m, "tff", step=3), 3) == [True]
    assert pd.combed_from_windows([[119, 500]], 3) == [False] and pd.combed_from_windows([[120, 120]], 3) == [True]
    assert pd.combed_from_windows([[39, 500], [40, 40]]) == [False, True] and pd.combed_from_windows([[39, 0]], pixels=39) == [True]
    rng = np.random.RandomState(1)
    for step in (1, 2, 3, 4):
        for r, c in ((9, 33), (17, 50), (20, 7)):
            for order in FIELD_ORDERS:
                v = rng.randint(0, 256, size=(2, r, c)) // 4
                assert np.array_equal(pd.comb_windows(v, order, step), _brute(v, order, step)), (step, r, c, order)


def test_depth_10_reads_the_8_most_significant_bits_and_clips():
    """Samples above 1023 count as 1023 (255 at the 8-bit scale): a 60000 between two 1023s is not combed."""
    m = np.full((1, 5, 8), 1023, np.int64)
    m[0, 1] = 60000
    assert pd.comb_windows(m, "tff", depth=10).tolist() == [[0, 0]]
    m[0, 3] = 0                                       # 0 between two 1023s: 255 + 255 at the 8-bit scale
    assert pd.comb_windows(m, "tff", depth=10).tolist() == [[8, 8]]
    m = np.zeros((1, 5, 8), np.int64)
    m[0, 1] = 43                                      # 43 >> 2 = 10: 2 * 10 = 20 > 18
    m[0, 3] = 39                                      # 39 >> 2 = 9: 18 is not
    assert pd.comb_windows(m, "tff", depth=10).tolist() == [[8, 8]]
    rng = np.random.RandomState(2)
    v = rng.randint(0, 5000, size=(2, 17, 33))
    for depth in (10, 12):
        assert np.array_equal(pd.comb_windows(v, "bff", 1, 9, depth), _brute(v, "bff", 1, 9, depth))


# ---------------------------------------------------------------------------------------------------------------------- clean film
def _clean_cases():
    for h, w in cc.SIZES:
        for kind in KINDS:
            for order in FIELD_ORDERS:
                yield kind, order, pd.telecine(packed_film(kind, 8, h, w), order), {}
    for fmt, layout, depth in (("i420", "420", 8), ("i422", "422", 10), ("y400", "400", 8)):
        for kind in KINDS:
            yield kind, "tff", pd.telecine(planar_film(kind, 8, 16, 16, depth, layout), "tff", 0, fmt, (16, 16), depth), dict(pixel_format=fmt, size=(16, 16), depth=depth)


def test_no_recovered_film_frame_is_flagged_so_combed_changes_nothing_on_clean_film():
    """The zero-flag condition: every woven frame of a cleanly recovered film reads 0 combed samples in its largest window (the gradient is
    vertically monotone, the bar vertically flat), so nothing is flagged and combed= returns the bytes and the info combed=None returns.
    The telecined bar's BC / CD frames do read combing (the gradient's 11-code step between film frames hardly passes the threshold), so
    the measure is not blind on these fixtures."""
    for kind, order, video, kw in _clean_cases():
        before = pd.frame_comb_windows(video, order, **kw)[:, 0]
        assert not before[[0, 1, 4, 5, 6, 9]].any() and (kind != "bar" or before[[2, 3, 7, 8]].min() >= 12), (kind, order, before)
        plain, pinfo = pd.remove_pulldown_frames(video, order, **kw)
        for method in DEINTERLACERS:
            film, info = pd.remove_pulldown_frames(video, order, combed=method, **kw)
            assert not info["comb"][:, 0].any() and info["combed"] == [], (kind, order, method)
            assert np.array_equal(film, plain) and info["kept"] == pinfo["kept"] and np.array_equal(info["sad"], pinfo["sad"])


def test_the_two_pixel_bar_stays_below_the_default_rule():
    """Small objects are not flagged: the bar's combing is two pixels wide, 32 pixels in a window at most."""
    for h, w in cc.SIZES:
        video = pd.telecine(packed_film("bar", 8, h, w), "tff")
        win = pd.frame_comb_windows(video, "tff")
        assert 0 < win[:, 0].max() <= 32 * 3 and not any(pd.combed_from_windows(win, 3))
        assert any(pd.combed_from_windows(win, 3, pixels=8))


# ---------------------------------------------------------------------------------------------------------------------- the hybrid
@pytest.mark.parametrize("method", DEINTERLACERS)
@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_hybrid_exactly_the_insert_is_flagged_and_comes_out_clean(order, method):
    for h, w in cc.SIZES:
        for fmt, depth in (("rgb", 8), ("i420", 8), ("i422", 10), ("y400", 8)):
            kw = {} if fmt == "rgb" else dict(pixel_format=fmt, size=(h, w), depth=depth)
            video, insert = cc.hybrid(order, h, w, fmt=fmt, depth=depth)
            assert video.shape[0] == 26 and insert == list(range(10, 16))
            film, info = pd.remove_pulldown_frames(video, order, combed=method, **kw)
            assert info["combed"] == insert and info["comb"].shape == (26, 2) and info["comb"].dtype == np.int64, (h, w, fmt)
            step = 3 if fmt == "rgb" else 1
            assert info["comb"][insert, 0].min() >= 40 * step and not np.delete(info["comb"][:, 0], insert).any()
            # the cleaned frames are the same-rate deinterlacer's, computed from the woven frames (not from cleaned ones)
            woven = pd.weave(video, order, info["matches"], **kw)
            clean = deinterlace_frames(woven, order, method=method, rate="same", **kw)
            cleaned = woven.copy()
            cleaned[insert] = clean[insert]
            assert np.array_equal(film, cleaned[info["kept"]])
            assert np.array_equal(pd.clean_combed(woven, order, [k in insert for k in range(26)], method, **kw), cleaned)
            # ... and nothing of the result is combed any more; without combed= the insert's kept frames still are
            assert not pd.frame_comb_windows(film, order, **kw).any(), (h, w, fmt)
            plain = pd.remove_pulldown_frames(video, order, **kw)[0]
            assert pd.frame_comb_windows(plain, order, **kw)[:, 0].max() >= 40 * step
            # the decimation read the cleaned frames
            assert np.array_equal(info["sad"][1:], pd.pair_sad(cleaned, **kw)) and film.shape[0] == 26 - 5


def test_a_stream_that_starts_inside_bc_cd_gets_its_leading_frame_cleaned():
    """Phase 3 starts at CD: frame 0's second field belongs to a film frame whose first field was cut off; the match can only keep it."""
    film = cc.packed("sinusoid", 8, 16, 32)
    video = pd.telecine(film, "tff", 3)
    plain, pinfo = pd.remove_pulldown_frames(video, "tff")
    assert pinfo["matches"][0] == 0 and pd.frame_comb_windows(plain[:1], "tff")[0, 0] >= 120          # kept, and combed
    out, info = pd.remove_pulldown_frames(video, "tff", combed="bwdif")
    assert info["combed"] == [0] and 0 in info["kept"]
    assert not pd.frame_comb_windows(out, "tff").any()
    assert np.array_equal(out[1:], plain[1:]) and not np.array_equal(out[0], plain[0])


def test_combed_none_runs_what_ran_before():
    video = cc.hybrid("tff", 16, 16)[0]
    a, ia = pd.remove_pulldown_frames(video, "tff")
    b, ib = pd.remove_pulldown_frames(video, "tff", combed=None)
    assert sorted(ia) == sorted(ib) == ["kept", "matches", "sad", "scores"] and np.array_equal(a, b)
    assert sorted(pd.remove_pulldown_frames(video, "tff", combed="yadif")[1]) == ["comb", "combed", "kept", "matches", "sad", "scores"]


def test_parameters_move_the_rule():
    video, insert = cc.hybrid("tff", 16, 16)
    assert pd.remove_pulldown_frames(video, "tff", combed="yadif", comb_threshold=255)[1]["combed"] == []
    assert pd.remove_pulldown_frames(video, "tff", combed="yadif", comb_pixels=128)[1]["combed"] == []       # 16 x 16 and tff: 7 scored rows
    assert pd.remove_pulldown_frames(video, "tff", combed="yadif", comb_pixels=1, comb_threshold=0)[1]["combed"] != insert


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_of_the_specification():
    m = np.zeros((1, 5, 8), np.int64)
    for bad in (0, 5, True, 1.0):
        with pytest.raises(ValueError, match="step = "):
            pd.comb_windows(m, "tff", step=bad)
    for bad in (-1, 256, 9.0, True):
        with pytest.raises(ValueError, match="threshold = "):
            pd.comb_windows(m, "tff", threshold=bad)
    with pytest.raises(ValueError, match=r"\[N, R, C\] integers"):
        pd.comb_windows(m.astype(np.float32), "tff")
    with pytest.raises(ValueError, match="one of tff, bff"):
        pd.comb_windows(m, "top")
    u8 = np.zeros((5, 4, 6, 3), np.uint8)
    with pytest.raises(ValueError, match="combed = 'weave': None or one of 'yadif', 'bwdif'"):
        pd.remove_pulldown_frames(u8, "tff", combed="weave")
    with pytest.raises(ValueError, match="comb_threshold = 10 goes with combed="):
        pd.remove_pulldown_frames(u8, "tff", comb_threshold=10)
    with pytest.raises(ValueError, match="comb_pixels = 30 goes with combed="):
        pd.remove_pulldown_frames(u8, "tff", comb_pixels=30)
    with pytest.raises(ValueError, match="comb_pixels = 0: an int in 1 .. 128"):
        pd.remove_pulldown_frames(u8, "tff", combed="yadif", comb_pixels=0)
    with pytest.raises(ValueError, match="comb_threshold = 256: an int in 0 .. 255"):
        pd.remove_pulldown_frames(u8, "tff", combed="yadif", comb_threshold=256)


def test_the_public_calls_refuse_before_the_gpu_is_needed():
    import savsr_amd
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.prepass import make_stage
    from savsr_amd.video import VideoUpscaler
    u8 = torch.zeros(10, 4, 6, 3, dtype=torch.uint8)
    net = SAVSR().eval()
    with pytest.raises(ValueError, match=r"combed = 'bwdif' goes with pulldown= \(or scan='detect'\)"):
        net.upscale_video(u8, combed="bwdif")
    with pytest.raises(ValueError, match="combed = 'yadif' together with fields = 'tff'"):
        net.upscale_video(u8, fields="tff", combed="yadif")
    with pytest.raises(ValueError, match="combed = 'yadif' together with fields = 'bff'"):
        VideoUpscaler(net, 2, fields="bff", combed="yadif")
    with pytest.raises(ValueError, match="combed = 'yadif' goes with pulldown="):
        VideoUpscaler(net, 2, combed="yadif")
    with pytest.raises(ValueError, match="comb_threshold = 12 goes with combed="):
        net.upscale_video(u8, pulldown="tff", comb_threshold=12)
    with pytest.raises(ValueError, match="comb_pixels = 41 goes with combed="):
        VideoUpscaler(net, 2, pulldown="tff", comb_pixels=41)
    with pytest.raises(ValueError, match="comb_pixels = 41 goes with combed="):
        net.upscale_video(u8, comb_pixels=41)
    with pytest.raises(ValueError, match="combed = 'blend': None or one of"):
        net.upscale_video(u8, pulldown="tff", combed="blend")
    with pytest.raises(ValueError, match="comb_pixels = 129: an int in 1 .. 128"):
        net.upscale_video(u8, pulldown="tff", combed="bwdif", comb_pixels=129)
    with pytest.raises(ValueError, match="combed = 'blend'"):
        savsr_amd.remove_pulldown(u8, "tff", combed="blend")
    with pytest.raises(ValueError, match="comb_threshold = -1: an int in 0 .. 255"):
        savsr_amd.remove_pulldown(u8, "tff", combed="yadif", comb_threshold=-1)
    with pytest.raises(ValueError, match="threshold = 300"):
        savsr_amd.comb_windows(u8, "tff", threshold=300)
    with pytest.raises(ValueError, match="float frames have no integer samples"):
        savsr_amd.comb_windows(torch.zeros(5, 3, 4, 6), "tff")
    with pytest.raises(TypeError):                    # keyword only
        savsr_amd.remove_pulldown(u8, "tff", "rgb", None, 8, 5, False, "yadif")
    # deinterlacer= with pulldown= stays refused exactly as it was: combed names its own method
    with pytest.raises(ValueError, match="deinterlacer = 'bwdif' together with pulldown = 'tff'"):
        net.upscale_video(u8, pulldown="tff", deinterlacer="bwdif", combed="bwdif")
    side_size = __import__("savsr_amd.frames", fromlist=["detector_side"]).detector_side("rgb", None, 8)
    stage = make_stage(None, "tff", 5, *side_size, combed="bwdif", comb_pixels=30)
    assert (stage.combed, stage.comb_threshold, stage.comb_pixels, stage.held) == ("bwdif", 9, 30, 0) and stage.info == {"matches": [], "kept": [], "combed": []}
    assert make_stage(None, "tff", 5, *side_size).info == {"matches": [], "kept": []}


def test_cli_arguments(tmp_path, capsys):
    from savsr_amd.upscale import parse_args
    base = ["-o", str(tmp_path / "out"), "--scale", "2", "--checkpoint", "net.pth"]
    a = parse_args(["-i", "in.y4m"] + base)
    assert a.combed is None and (a.comb_threshold, a.comb_pixels) == (9, 40)
    a = parse_args(["-i", "in.y4m", "--pulldown", "tff", "--combed", "bwdif", "--comb-threshold", "12", "--comb-pixels", "30"] + base)
    assert (a.combed, a.comb_threshold, a.comb_pixels) == ("bwdif", 12, 30)
    assert parse_args(["-i", "in.y4m", "--pulldown", "auto", "--combed", "none"] + base).combed is None
    assert parse_args(["-i", "in.y4m", "--scan", "detect", "--combed", "yadif"] + base).combed == "yadif"
    assert parse_args(["-i", "in.y4m", "--combed", "none"] + base).combed is None
    for extra, words in ((["-i", "in.y4m", "--combed", "yadif"], "--combed yadif goes with --pulldown"),
                         (["-i", "in.y4m", "--pulldown", "none", "--combed", "bwdif"], "--combed bwdif goes with --pulldown"),
                         (["-i", "in.y4m", "--fields", "tff", "--combed", "bwdif"], "--combed bwdif goes with --pulldown"),
                         (["-i", "in.y4m", "--pulldown", "tff", "--comb-threshold", "12"], "go with --combed"),
                         (["-i", "in.y4m", "--pulldown", "tff", "--combed", "none", "--comb-pixels", "12"], "go with --combed"),
                         (["-i", "in.y4m", "--pulldown", "tff", "--combed", "yadif", "--comb-pixels", "0"], "--comb-pixels = 0: an int in 1 .. 128"),
                         (["-i", "in.y4m", "--pulldown", "tff", "--combed", "yadif", "--comb-threshold", "256"], "--comb-threshold = 256"),
                         (["-i", "in.y4m", "--pulldown", "tff", "--combed", "blend"], "invalid choice")):
        with pytest.raises(SystemExit):
            parse_args(extra + base)
        assert words in capsys.readouterr().err, extra
