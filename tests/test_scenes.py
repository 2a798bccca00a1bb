"""Scene cuts, host side (no GPU): the segment windows against a direct restatement, the numpy specification of the detector's scores on
hand-made frames, scdet's rule at its boundary, the streaming plan with cuts revealed as frames arrive, refusals and the CLI's arguments."""
import random
from fractions import Fraction

import numpy as np
import pytest
import torch

from savsr_amd import scenes
from savsr_amd.harness import window_indices
from savsr_amd.video import PADDING_MODES, check_length, window_lists
from savsr_amd.yuv import i420_bytes

T = 7


def _random_cuts(rng, n):
    if n < 2:
        return []
    return sorted(rng.sample(range(1, n), rng.randint(0, min(n - 1, 6))))


def _restated(n, cuts, num_frame, padding):
    """The definition, written out: every segment alone, shifted by its start, "replicate" exactly when check_length refuses it."""
    out = []
    edges = [0] + list(cuts) + [n]
    for a, b in zip(edges[:-1], edges[1:]):
        try:
            check_length(b - a, num_frame, padding)
            mode = padding
        except ValueError:
            mode = "replicate"
        for i in range(b - a):
            out.append([a + j for j in window_indices(i, b - a, num_frame, mode)])
    return out


# ------------------------------------------------------------------------------------------------------------------------- windows
@pytest.mark.parametrize("padding", PADDING_MODES)
def test_scene_windows_are_the_segments_windows(padding):
    rng = random.Random(PADDING_MODES.index(padding))
    fell_back = kept = 0
    for n in range(1, 31):
        for _ in range(12):
            cuts = _random_cuts(rng, n)
            got = scenes.scene_windows(n, cuts, T, padding)
            assert got == _restated(n, cuts, T, padding), (n, cuts)
            assert len(got) == n
            for (a, b) in scenes.segments(n, cuts):
                for i in range(a, b):
                    assert a <= min(got[i]) and max(got[i]) < b and got[i][T // 2] == i        # a window never leaves its segment
                mode = scenes.segment_mode(b - a, T, padding)
                fell_back += mode != padding
                kept += mode == padding
    assert kept > 0 and (fell_back > 0 or padding == "replicate")


@pytest.mark.parametrize("padding", PADDING_MODES)
@pytest.mark.parametrize("num_frame", [3, 5, 7, 9])
def test_segment_mode_is_check_lengths_decision(padding, num_frame):
    for length in range(1, 4 * num_frame):
        try:
            check_length(length, num_frame, padding)
            want = padding
        except ValueError:
            want = "replicate"
        assert scenes.segment_mode(length, num_frame, padding) == want, length
    check_length(scenes.min_length(num_frame, padding), num_frame, padding)
    check_length(1, num_frame, "replicate")


@pytest.mark.parametrize("padding", PADDING_MODES)
def test_no_cuts_is_window_lists(padding):
    for n in range(scenes.min_length(T, padding), 31):
        assert scenes.scene_windows(n, [], T, padding) == window_lists(n, T, padding)


def test_a_short_video_is_served_once_cuts_are_given():
    with pytest.raises(ValueError, match="too few"):
        window_lists(3, T, "circle")
    assert scenes.scene_windows(3, [], T, "circle") == [window_indices(i, 3, T, "replicate") for i in range(3)]
    assert scenes.scene_windows(1, [], T, "reflection") == [[0] * T]


# ---------------------------------------------------------------------------------------------------------------------- the scores
def test_pair_sad_u8_known_sums():
    for (h, w, c) in [(5, 3, 3), (7, 9, 1), (2, 2, 2), (181, 319, 3)]:
        f = np.zeros((4, h, w, c), np.uint8)
        f[1] = 255                                             # 0 -> 255: the largest change
        f[2] = 255
        f[2, 0, 0, 0] = 250                                    # one sample by 5
        f[3] = f[2]
        f[3, h - 1, w - 1, c - 1] -= 7                         # the last byte by 7
        got = scenes.pair_sad(f)
        assert got.dtype == np.int64 and got.tolist() == [255 * h * w * c, 5, 7]
        assert scenes.sad_samples(f.shape) == h * w * c
    assert scenes.pair_sad(np.zeros((1, 5, 3, 3), np.uint8)).shape == (0,)
    assert scenes.pair_sad(torch.zeros(2, 5, 3, 3, dtype=torch.uint8)).tolist() == [0]


def test_pair_sad_i420_reads_the_y_plane_only():
    h, w = 5, 3
    f = np.zeros((3, i420_bytes(h, w)), np.uint8)
    f[1, :h * w] = 9                   # Y
    f[1, h * w:] = 200                 # chroma: not compared
    f[2, :h * w] = 9
    f[2, h * w - 1] = 0
    assert scenes.pair_sad(f, "i420", (h, w)).tolist() == [9 * h * w, 9]
    assert scenes.sad_samples(f.shape, "i420", (h, w)) == h * w
    with pytest.raises(ValueError, match="I420 frames"):
        scenes.pair_sad(f[:, :-1], "i420", (h, w))
    with pytest.raises(ValueError, match="size"):
        scenes.pair_sad(f, "i420")


def test_pair_sad_float_quantises_like_the_uint8_output():
    # ties at k + 0.5 go to the even neighbour; values outside [0, 1] clamp; NaN -> 0
    ties = np.array([0.5, 1.5, 2.5, 3.5, 126.5, 127.5, 253.5, 254.5], np.float32) / np.float32(255)
    prod = ties * np.float32(255)
    want = np.rint(prod).astype(np.int64)                       # (whatever the float32 product is, rintf of it is the rule)
    for t, p, q in zip(ties, prod, want):
        if p == np.floor(p) + 0.5:                              # an exact tie in float32: round half to even
            assert q % 2 == 0, (t, p, q)
    assert scenes.quantize_u8(ties).tolist() == want.tolist()
    assert scenes.quantize_u8(np.array([-3.0, -0.0, 0.0, 1.0, 1.0001, 7.0, np.nan, np.inf, -np.inf], np.float32)).tolist() == \
        [0, 0, 0, 255, 255, 255, 0, 255, 0]
    assert scenes.quantize_u8(np.array([0.5 / 255, 1.5 / 255, 2.5 / 255])).tolist() == \
        np.rint((np.array([0.5 / 255, 1.5 / 255, 2.5 / 255]).astype(np.float32)) * np.float32(255)).astype(int).tolist()
    f = np.zeros((3, 2, 5, 3), np.float32)                      # [N, c, h, w]
    f[1] = 2.0                                                  # clamps to 255
    f[2] = 2.0
    f[2, 1, 4, 2] = np.nan                                      # -> 0
    f[2, 0, 0, 0] = -1.0                                        # -> 0
    f[2, 0, 0, 1] = 100.0 / 255.0
    assert scenes.pair_sad(f).tolist() == [255 * 30, 255 + 255 + 155]
    assert scenes.sad_samples(f.shape) == 30
    u8 = np.random.RandomState(3).randint(0, 256, (4, 6, 7, 3), dtype=np.uint8)      # k / 255 quantises back to k
    fl = (u8.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2)
    assert scenes.pair_sad(fl).tolist() == scenes.pair_sad(u8).tolist()


# ------------------------------------------------------------------------------------------------------------------------- the rule
def test_cuts_from_sad_is_exact_at_the_boundary():
    S = 5 * 3 * 3
    for thr in (10.0, 10, Fraction(1, 3), 0.1, 37.5):
        bound = Fraction(thr) * 255 * S / 100                   # m >= bound
        m = -(-bound.numerator // bound.denominator)            # the smallest integer that is a cut
        assert scenes.cuts_from_sad([m], S, thr) == [1]
        assert scenes.cuts_from_sad([m - 1], S, thr) == []
    # exactly on the boundary: 10 % of 255 * 40 samples = 1020
    assert scenes.cuts_from_sad([1020], 40, 10) == [1] and scenes.cuts_from_sad([1019], 40, 10) == []
    # 255 * 3 * H * W overflows 32 bits from 2.8 Mpixel on: Python ints all the way
    S = 3 * 4096 * 4096
    assert scenes.cuts_from_sad([255 * S, 255 * S], S, 100) == [1]
    assert scenes.cuts_from_sad(np.array([255 * S], np.int64), S, 100) == [1]


def test_cuts_from_sad_first_pair_sustained_motion_and_flash():
    S, X = 100, 255 * 100 // 2                                  # X: half of the largest change, far above 10 %
    assert scenes.cuts_from_sad([X], S) == [1]                  # the pair before frame 1 does not exist: its score is 0
    assert scenes.cuts_from_sad([X] * 6, S) == [1]              # sustained motion fires at its start only (|X - X| = 0 afterwards)
    assert scenes.cuts_from_sad([0, 0, X, X, X, 0, 0], S) == [3]
    assert scenes.cuts_from_sad([0, X, X, 0], S) == [2]         # A A B A A: once, at B; B travels with the frames after it
    assert scenes.cuts_from_sad([0, X, 0, 0, X, 0], S) == [2, 5]
    assert scenes.cuts_from_sad([], S) == []
    # streaming: the same decisions when the scores arrive in pieces, the last score carried over
    sad = [0, X, X, 0, X, 3, X, X]
    whole = scenes.cuts_from_sad(sad, S)
    for cut_at in range(1, len(sad)):
        a = scenes.cuts_from_sad(sad[:cut_at], S)
        b = scenes.cuts_from_sad(sad[cut_at:], S, first=1 + cut_at, prev=sad[cut_at - 1])
        assert a + b == whole, cut_at


# ------------------------------------------------------------------------------------------------------------------------ streaming
@pytest.mark.parametrize("padding", PADDING_MODES)
def test_streaming_plan_returns_only_settled_windows_and_keeps_what_is_needed(padding):
    """The plan behind VideoUpscaler(cuts=...), driven without an engine: cuts are revealed only with the frames that contain them, the
    chunking is random.  Every returned window is scene_windows' of the final video, names only frames pushed and still kept, and the
    kept span stays within num_frame - 1 past frames (num_frame in the circle modes)."""
    bound = T if "circle" in padding else T - 1
    for seed in range(250):
        rng = random.Random(seed * 7 + len(padding))
        n = rng.randint(1, 45)
        cuts = _random_cuts(rng, n)
        final = scenes.scene_windows(n, cuts, T, padding)
        plan = scenes.ScenePlan(T, padding)
        got, base, pos = [], 0, 0
        while pos < n:
            k = rng.randint(1, min(n - pos, rng.choice((1, 2, 5, 16))))
            plan.push(k, [c for c in cuts if max(pos, 1) <= c < pos + k])
            pos += k
            first = plan.done
            wins = plan.take()
            for i, win in enumerate(wins, first):
                assert win == final[i], (padding, n, cuts, i)
                assert base <= min(win) and max(win) < pos, (padding, n, cuts, i, base, pos)
            got += wins
            lo = plan.keep_from()
            assert base <= lo <= pos and pos - lo <= bound, (padding, n, cuts, pos, lo)
            base = lo
        assert plan.cuts == cuts
        plan.end()
        wins = plan.take()
        for win in wins:
            assert base <= min(win) and max(win) < n
        got += wins
        assert got == final and plan.done == n, (padding, n, cuts)


def test_streaming_plan_waits_for_what_can_still_change():
    plan = scenes.ScenePlan(T, "reflection")
    plan.push(3)
    assert plan.take() == []                       # 3 frames: neither the mode (4 needed) nor any right edge is settled
    plan.push(1)
    assert plan.take() == [[3, 2, 1, 0, 1, 2, 3]]  # 4 frames: frame 0 is interior on its right for every end >= 4
    plan.push(1, [4])                              # a cut at 4 closes [0, 4): its frames are known at once
    assert plan.take() == [[2, 1, 0, 1, 2, 3, 2], [1, 0, 1, 2, 3, 2, 1], [0, 1, 2, 3, 2, 1, 0]]
    plan.end()                                     # [4, 5): one frame, "replicate"
    assert plan.take() == [[4] * T]
    with pytest.raises(ValueError):
        scenes.ScenePlan(T, "reflection").push(4, [4])
    with pytest.raises(ValueError):
        scenes.ScenePlan(T, "reflection").push(4, [2, 2])


# ------------------------------------------------------------------------------------------------------------------------- refusals
def test_check_cuts_refusals():
    assert scenes.check_cuts([], 5) == [] and scenes.check_cuts((1, 4), 5) == [1, 4]
    assert scenes.check_cuts(np.array([2, 3]), 5) == [2, 3]
    for bad in ([0], [5], [6], [-1], [2, 2], [3, 2], [1.5], [True], ["2"]):
        with pytest.raises(ValueError):
            scenes.check_cuts(bad, 5)
    for bad in ("auto", "1,2", 3, None):
        with pytest.raises(ValueError):
            scenes.check_cuts(bad, 5)
    assert scenes.check_cuts([7], None) == [7]                  # the length is not known yet
    with pytest.raises(ValueError):
        scenes.scene_windows(5, [5], T, "reflection")
    with pytest.raises(ValueError, match="no frames"):
        scenes.scene_windows(0, [], T, "reflection")
    with pytest.raises(ValueError, match="generate_frame_indices"):
        scenes.scene_windows(5, [], T, "zero")


def test_threshold_refusals():
    assert scenes.check_threshold(10.0) == 10 and scenes.check_threshold(Fraction(1, 3)) == Fraction(1, 3)
    for bad in (0, 0.0, -1, float("nan"), float("inf"), "10", None, True):
        with pytest.raises(ValueError):
            scenes.check_threshold(bad)
        with pytest.raises(ValueError):
            scenes.cuts_from_sad([1], 10, bad)


class _Net:
    """What upscale_video / VideoUpscaler read before they touch the GPU."""
    training = False
    cfg = {"num_in_ch": 3}
    scale = (4.0, 4.0)
    num_frame = T
    self_ensemble = False
    gamma = torch.zeros(1)


def test_entry_points_refuse_bad_cuts_before_the_gpu():
    from savsr_amd import VideoUpscaler
    from savsr_amd.video import upscale_video
    v = torch.zeros(6, 8, 8, 3, dtype=torch.uint8)
    for bad in ([0], [6], [3, 3], [4, 2], "scenes", "AUTO", [1.0], 3):
        with pytest.raises(ValueError):
            upscale_video(_Net(), v, cuts=bad)
    for bad in ([0], [3, 3], [4, 2], "scenes", [1.0]):
        with pytest.raises(ValueError):
            VideoUpscaler(_Net(), cuts=bad)
    for thr in (0, -2.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError):
            upscale_video(_Net(), v, cuts="auto", scene_threshold=thr)
        with pytest.raises(ValueError):
            VideoUpscaler(_Net(), cuts="auto", scene_threshold=thr)
    with pytest.raises(ValueError, match="too few"):            # no cuts: refused as before
        upscale_video(_Net(), v[:3], padding="reflection")
    with pytest.raises(RuntimeError, match="AMD GPU"):          # with cuts the short video passes the host checks
        upscale_video(_Net(), v[:3], padding="reflection", cuts=[])
    with pytest.raises(RuntimeError, match="AMD GPU"):
        upscale_video(_Net(), v, cuts=np.array([2, 4]))
    up = VideoUpscaler(_Net(), cuts=[2, 9])
    assert up.cuts == [] and VideoUpscaler(_Net()).cuts is None


def test_detector_entry_points_check_their_arguments():
    import savsr_amd
    v = torch.zeros(3, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        savsr_amd.detect_cuts(v, threshold=0)
    with pytest.raises(ValueError):
        savsr_amd.detect_cuts(v, pixel_format="nv12")
    with pytest.raises(ValueError):
        savsr_amd.pair_sad(v, pixel_format="i420")
    with pytest.raises(ValueError):
        savsr_amd.pair_sad(torch.zeros(3, 4, 4, 4, dtype=torch.uint8))           # 4 channels
    with pytest.raises(ValueError):
        savsr_amd.pair_sad(torch.zeros(3, 3, 4, 4))                               # float frames on the host
    with pytest.raises(ValueError):
        savsr_amd.pair_sad(torch.zeros(0, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(TypeError):
        savsr_amd.pair_sad(np.zeros((3, 4, 4, 3), np.uint8))


# ------------------------------------------------------------------------------------------------------------------------------ CLI
def test_cli_cut_arguments(tmp_path):
    from savsr_amd.upscale import parse_args
    base = ["-i", "in", "-o", "out", "--scale", "4", "--checkpoint", "x.pth"]
    a = parse_args(base)
    assert a.cuts is None and a.cuts_out is None and a.scene_threshold == 10.0
    a = parse_args(base + ["--cuts", "auto", "--scene-threshold", "7.5", "--cuts-out", "c.txt"])
    assert a.cuts == "auto" and a.scene_threshold == 7.5 and a.cuts_out == "c.txt"
    assert parse_args(base + ["--cuts", "3,10, 24"]).cuts == [3, 10, 24]
    lst = tmp_path / "cuts.txt"
    lst.write_text("5\n\n17\n40\n")
    assert parse_args(base + ["--cuts", f"@{lst}"]).cuts == [5, 17, 40]
    (tmp_path / "none.txt").write_text("")
    assert parse_args(base + ["--cuts", f"@{tmp_path / 'none.txt'}"]).cuts == []
    for bad in (["--cuts", "0"], ["--cuts", "5,3"], ["--cuts", "4,4"], ["--cuts", "a,b"], ["--cuts", ""], ["--cuts", "detect"],
                ["--cuts", f"@{tmp_path / 'missing.txt'}"], ["--cuts", "auto", "--scene-threshold", "0"],
                ["--cuts", "auto", "--scene-threshold", "nan"], ["--cuts-out", "c.txt"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
