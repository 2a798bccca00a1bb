"""Scan detection on the host: savsr_amd/scan.py, the numpy specification of field_stats (csrc/scan.hip) and the decision rule on its
sums; the streaming accumulator's bookkeeping; the refusals of the public calls and of the command line that need no GPU."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from savsr_amd import pulldown as pd
from savsr_amd import scan as sc
from savsr_amd.deinterlace import FIELD_FLAGS, FIELD_ORDERS
from tests.scan_cases import MOTIONS, NOISES, PHASES, SIZES, expected, matrix_case, noise_mats, packed_case, planar_case


# ---------------------------------------------------------------------------------------------------------------------- field_stats
def _literal(m, depth=8):
    """The definition in three loops."""
    top, shift = (1 << depth) - 1, depth - 8
    N, R, C = m.shape

    def s(n, y, x):
        return min(int(m[n, y, x]), top) >> shift

    def comb(a, b, c):
        return abs(a - b) + abs(c - b) - abs(a - c)

    out = np.zeros((N, 8), np.int64)
    for n in range(N):
        prev, nxt = max(n - 1, 0), min(n + 1, N - 1)
        for y in range(R):
            q = y % 2
            for x in range(C):
                out[n, 6 + q] += abs(s(n, y, x) - s(prev, y, x))
                if 1 <= y <= R - 2:
                    a, c = s(n, y - 1, x), s(n, y + 1, x)
                    out[n, 0 + q] += comb(a, s(prev, y, x), c)
                    out[n, 2 + q] += comb(a, s(nxt, y, x), c)
                    out[n, 4 + q] += comb(a, s(n, y, x), c)
    return out


@pytest.mark.parametrize("r", [1, 2, 3, 4, 7])
@pytest.mark.parametrize("c", [1, 5])
def test_field_stats_equal_the_literal_definition(r, c):
    for n in (1, 2, 4):
        m = noise_mats(n, r, c, 255, seed=10 * r + c + n)
        got = sc.field_stats(m)
        assert got.dtype == np.int64 and got.shape == (n, 8) and np.array_equal(got, _literal(m))
        assert (got >= 0).all()
        if r < 3:
            assert not got[:, :6].any()                                              # no row between two others
        if r == 1:
            assert not got[:, 7].any()                                               # no row of parity 1
    m = noise_mats(3, 5, 4, 4095, seed=3)
    assert np.array_equal(sc.field_stats(m, 12), _literal(m, 12)) and np.array_equal(sc.field_stats(m, 10), _literal(m, 10))


@pytest.mark.parametrize("depth", [8, 10, 12])
@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_field_stats_hold_the_field_scores(order, depth):
    """comb_prev[1 - p] and comb_self[1 - p] are pulldown.field_scores' two candidates."""
    p = pd.first_parity(order)
    for r, c in ((2, 3), (3, 4), (8, 5), (9, 16)):
        m = noise_mats(5, r, c, (1 << depth) - 1, seed=r + c + depth)
        st, fs = sc.field_stats(m, depth), pd.field_scores(m, order, depth)
        assert np.array_equal(st[:, 0 + 1 - p], fs[:, 0]) and np.array_equal(st[:, 4 + 1 - p], fs[:, 1])


@pytest.mark.parametrize("depth", [10, 12])
def test_samples_above_the_depth_are_clamped(depth):
    top = (1 << depth) - 1
    m = noise_mats(3, 6, 7, top, seed=depth)
    over = m.copy()
    over[m == top] = 65535
    over[0, 0, 0], m[0, 0, 0] = 40000, top
    assert (over > top).any() and np.array_equal(sc.field_stats(over.astype(np.uint16), depth), sc.field_stats(m, depth))


def test_frame_stats_read_every_byte_of_packed_frames_and_the_y_plane_of_planar_ones():
    v = np.random.RandomState(1).randint(0, 256, size=(4, 6, 5, 3), dtype=np.uint8)
    assert np.array_equal(sc.frame_stats(v), sc.field_stats(v.reshape(4, 6, 15)))
    assert np.array_equal(sc.frame_stats(torch.from_numpy(v)), sc.frame_stats(v))
    h, w = 6, 10
    yv = np.random.RandomState(2).randint(0, 256, size=(4, h * w * 3 // 2), dtype=np.uint8)
    assert np.array_equal(sc.frame_stats(yv, "i420", (h, w)), sc.field_stats(yv[:, :h * w].reshape(4, h, w)))
    with pytest.raises(ValueError, match="float frames have no integer samples"):
        sc.frame_stats(np.zeros((3, 4, 5, 3), np.float32))
    with pytest.raises(ValueError, match=r"\[N, R, C\] integers"):
        sc.field_stats(np.zeros((3, 4, 5), np.float32))
    with pytest.raises(ValueError, match=r"\[N, R, C\] integers"):
        sc.field_stats(np.zeros((4, 5), np.uint8))


# ---------------------------------------------------------------------------------------------------------------------- the decision
def _verdict(m, **kw):
    return sc.verdict_from_stats(sc.field_stats(m), **kw)


CASES = [("progressive", None, 0), ("interlaced", "tff", 0), ("interlaced", "bff", 0)] + [("telecine", o, ph) for o in FIELD_ORDERS for ph in PHASES]


@pytest.mark.parametrize("noise", NOISES)
@pytest.mark.parametrize("motion", MOTIONS)
@pytest.mark.parametrize("size", SIZES)
def test_verdicts_on_smooth_moving_pictures(size, motion, noise):
    r, c = size
    for kind, order, phase in CASES:
        v = _verdict(matrix_case(kind, order, r, c, motion=motion, noise=noise, phase=phase))
        assert (v.scan, v.order) in expected(kind, order), (kind, order, phase, v)
        assert v.scan in sc.SCANS and len(v.rep_field) == (13 if kind == "telecine" else 12)
        if kind == "telecine":
            p = pd.first_parity(order)
            assert v.hits[p] >= 2 and v.hits[1 - p] == 0


def test_the_repeated_fields_of_aa_bb_bc_cd_dd():
    """Phase 0: the third frame of every cycle repeats its first field, the fifth its second."""
    for order in FIELD_ORDERS:
        p = pd.first_parity(order)
        v = _verdict(matrix_case("telecine", order, 12, 20, motion=(2, 1)))
        assert list(v.rep_field[:10]) == [None, None, p, None, 1 - p, None, None, p, None, 1 - p]


def test_static_short_and_duplicate_videos():
    for r, c in SIZES:
        v = _verdict(matrix_case("static", None, r, c))
        assert (v.scan, v.order, v.kwargs()) == ("undetermined", None, {}) and v.rep_field == (None,) * 12 and v.hits == (0, 0)
        assert (v.s, v.a_tff, v.a_bff) == (v.s, v.s, v.s)                            # every field fits as the frame's own does
    for n in (0, 1, 2):                                                              # N < 3: no frame has two real neighbours
        m = matrix_case("interlaced", "tff", 12, 20)[:n]
        v = _verdict(m)
        assert v.scan == "undetermined" and (v.s, v.a_tff, v.a_bff) == (0, 0, 0) and len(v.rep_field) == n
    assert _verdict(matrix_case("interlaced", "tff", 12, 20)[:3]).scan == "interlaced"
    # exact duplicates: rep is 0 for both fields and 3 * 0 < 0 is false, so a duplicated frame repeats nothing
    dup = np.repeat(matrix_case("progressive", None, 12, 20, motion=(2, 1))[:6], 2, 0)
    v = _verdict(dup)
    assert v.rep_field == (None,) * 12 and v.hits == (0, 0) and v.scan != "telecine"
    flat = np.full((12, 9, 17), 77, np.uint8)
    assert _verdict(flat).scan == "undetermined"


def test_thresholds_decide_exactly():
    """Hand-made rows: the comparisons are strict and exact."""
    def rows(a_tff, a_bff, s, n=3):
        st = np.zeros((n, 8), np.int64)
        st[1] = [a_tff, a_bff, 0, 0, s, 0, 5, 5]
        return st
    assert sc.verdict_from_stats(rows(15, 15, 10)).scan == "undetermined"            # min(A) = 3/2 S: not above
    assert sc.verdict_from_stats(rows(16, 16, 10)).scan == "progressive"
    v = sc.verdict_from_stats(rows(5, 4, 10))                                        # 5 = 5/4 * 4: not above
    assert (v.scan, v.s, v.a_tff, v.a_bff) == ("undetermined", 10, 5, 4)
    assert sc.verdict_from_stats(rows(6, 4, 10)).kwargs() == {"fields": "tff"}
    assert sc.verdict_from_stats(rows(4, 6, 10)).kwargs() == {"fields": "bff"}
    assert sc.verdict_from_stats(rows(5, 4, 10), interlace_threshold=1.125).order == "tff"
    assert sc.verdict_from_stats(rows(16, 16, 10), progressive_threshold=Fraction(8, 5)).scan == "undetermined"
    big = rows(3 * 2 ** 61, 2 ** 62, 2 ** 62)                                           # int64 sums compared as Python integers
    assert sc.verdict_from_stats(big).order == "tff"
    st = np.zeros((5, 8), np.int64)
    st[:, 6:] = [[0, 0], [1, 3], [1, 4], [4, 1], [3, 1]]
    assert sc.verdict_from_stats(st).rep_field == (None, None, 0, 1, None)           # 3 * 1 < 3 is false
    assert sc.verdict_from_stats(st, repeat_threshold=2).rep_field == (None, 0, 0, 1, 1)
    with pytest.raises(ValueError, match=r"\[N, 8\] integers"):
        sc.verdict_from_stats(np.zeros((3, 2), np.int64))


def test_the_telecine_rule_counts_hits():
    def stats(fields):
        st = np.zeros((len(fields), 8), np.int64)
        for n, q in enumerate(fields):
            if q is not None:
                st[n, 6 + q], st[n, 7 - q] = 1, 100
        return st
    cad = [None, None, 0, None, 1]
    v = sc.verdict_from_stats(stats(cad * 3))
    assert (v.scan, v.order, v.hits) == ("telecine", "tff", (3, 0)) and v.kwargs() == {"pulldown": "tff"}
    v = sc.verdict_from_stats(stats([None, None, 1, None, 0] * 3))
    assert (v.scan, v.order, v.hits) == ("telecine", "bff", (0, 3))
    assert sc.verdict_from_stats(stats(cad + [None] * 5 + cad)).scan == "telecine"  # 2 of 3 cycles show it: 10 * 2 >= 15 - 3
    assert sc.verdict_from_stats(stats(cad + [None] * 5)).scan != "telecine"         # one hit is no cadence
    assert sc.verdict_from_stats(stats(cad * 2)).hits == (2, 0)
    long = stats(cad * 2 + [None] * 14)                                              # 2 hits in 24 frames: 20 < 21, the cadence is the exception
    assert sc.verdict_from_stats(long).hits == (2, 0) and sc.verdict_from_stats(long).scan != "telecine"
    assert sc.verdict_from_stats(stats([None, 0, None, 1, None, 1, None, 0, None, None])).hits == (1, 1)           # a tie is no cadence
    assert sc.verdict_from_stats(stats([None, 0, None, 1, None, 1, None, 0, None, None])).scan != "telecine"
    assert sc.verdict_from_stats(stats([0, None, 1, None, None])).hits == (0, 0)     # frame 0 has no predecessor


def test_threshold_arguments_are_checked():
    st = np.zeros((4, 8), np.int64)
    for name in ("interlace_threshold", "progressive_threshold", "repeat_threshold"):
        for bad, words in ((True, "positive number"), ("2", "positive number"), (None, "positive number"), (float("nan"), "finite"),
                           (float("inf"), "finite"), (0, "positive"), (-1.5, "positive")):
            with pytest.raises(ValueError, match=f"{name} must be .*{words}"):
                sc.verdict_from_stats(st, **{name: bad})
        for good in (2, 1.5, Fraction(7, 3)):
            assert getattr(sc.verdict_from_stats(st, **{name: good}), name) == Fraction(good)
    v = sc.verdict_from_stats(st)
    assert (v.interlace_threshold, v.progressive_threshold, v.repeat_threshold) == (Fraction(5, 4), Fraction(3, 2), Fraction(3))


def test_kwargs_flags_and_json():
    def v(scan, order):
        return sc.ScanVerdict(scan, order, 1, 2, 3, (4, 5), (None, 0, 1))
    assert v("interlaced", "tff").kwargs() == {"fields": "tff"} and v("interlaced", "bff").flag() == "--fields bff"
    assert v("telecine", "bff").kwargs() == {"pulldown": "bff"} and v("telecine", "bff").flag() == "--pulldown bff"
    assert v("telecine", "bff").describe() == "telecine, bottom field first" and v("interlaced", "tff").describe() == "interlaced, top field first"
    for scan in ("progressive", "undetermined"):
        assert v(scan, None).kwargs() == {} and v(scan, None).flag() is None and v(scan, None).describe() == scan
    j = v("telecine", "tff").as_json()
    assert j["scan"] == "telecine" and j["order"] == "tff" and j["totals"] == {"S": 1, "A_tff": 2, "A_bff": 3}
    assert j["hits"] == [4, 5] and j["rep_field"] == [None, 0, 1] and j["thresholds"]["interlace"] == "5/4"
    # the note about a tag that says something else
    assert sc.tag_note(v("interlaced", "tff"), "t") is None and sc.tag_note(v("telecine", "bff"), "b") is None
    assert sc.tag_note(v("progressive", None), "p") is None and sc.tag_note(v("interlaced", "tff"), None) is None
    assert sc.tag_note(v("undetermined", None), "t") is None
    assert "tagged Ip, its content is interlaced, top field first" in sc.tag_note(v("interlaced", "tff"), "p")
    assert "tagged It, its content is progressive" in sc.tag_note(v("progressive", None), "t")
    assert "tagged It" in sc.tag_note(v("telecine", "bff"), "t") and "tagged I?" in sc.tag_note(v("interlaced", "bff"), "?")


def test_detect_scan_frames_on_packed_and_planar_frames():
    for kind, order in (("interlaced", "tff"), ("interlaced", "bff"), ("telecine", "bff"), ("progressive", None)):
        v = sc.detect_scan_frames(packed_case(kind, order, 12, 20, motion=(2, 1)))
        assert (v.scan, v.order) in expected(kind, order)
        for depth in (8, 10):
            frames = planar_case(kind, order, 12, 20, depth, motion=(2, 1))
            v = sc.detect_scan_frames(frames, "i420", (12, 20), depth)
            assert (v.scan, v.order) in expected(kind, order), (kind, order, depth)


# ---------------------------------------------------------------------------------------------------------------------- streaming
@pytest.mark.parametrize("chunks", [(1,) * 7, (2, 3, 1, 1), (7,), (1, 6), (3, 0, 4)])
def test_scan_stats_bookkeeping_on_a_stubbed_stats_function(chunks):
    """ScanStats with the numpy specification in the kernel's place: any chunking gives field_stats on the whole video, the last frame
    is held back and at most two frames are kept."""
    from savsr_amd.frames import detector_side
    from savsr_amd.prepass import ScanStats
    frames = torch.from_numpy(np.random.RandomState(4).randint(0, 256, size=(7, 6, 5, 3), dtype=np.uint8))
    calls = []

    def stub(src, side, size, lo, hi):
        calls.append((int(src.shape[0]), lo, hi))
        return torch.from_numpy(sc.frame_stats(src.numpy()))[lo:hi] if hi > lo else torch.zeros(0, 8, dtype=torch.int64)

    acc = ScanStats(*detector_side("rgb", None, 8), stats=stub)
    assert acc.finish() is None
    acc = ScanStats(*detector_side("rgb", None, 8), stats=stub)
    parts, a, done = [], 0, 0
    for k in chunks:
        parts.append(acc.push(frames[a:a + k]))
        a += k
        done += int(parts[-1].shape[0])
        assert acc.seen == a and done == max(a - 1, 0) and acc.held <= max(2, k if done == 0 else 2)
    last = acc.finish()
    assert last.shape == (1, 8) and acc.held == 0 and acc.finish() is None
    assert np.array_equal(torch.cat(parts + [last], 0).numpy(), sc.frame_stats(frames.numpy()))
    assert all(n <= 2 + k for (n, _, _), k in zip(calls, chunks))                    # the context, the held frame and the chunk


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_the_public_calls_refuse_before_the_gpu_is_needed():
    import savsr_amd
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.video import VideoUpscaler, _check_scan
    u8 = torch.zeros(10, 4, 6, 3, dtype=torch.uint8)
    assert _check_scan(None, "tff", None, 5) is None and _check_scan(None, None, "bff", 4) is None and _check_scan("detect", None, None, 5) == "detect"
    assert savsr_amd.ScanVerdict is sc.ScanVerdict and savsr_amd.scan is sc
    with pytest.raises(ValueError, match="float frames have no integer samples"):
        savsr_amd.field_stats(torch.zeros(5, 3, 4, 6))
    with pytest.raises(ValueError, match="float frames have no integer samples"):
        savsr_amd.detect_scan(torch.zeros(5, 3, 4, 6))
    with pytest.raises(ValueError, match="interlace_threshold must be positive"):
        savsr_amd.detect_scan(u8, interlace_threshold=0)
    with pytest.raises(ValueError, match="repeat_threshold must be a positive number"):
        savsr_amd.detect_scan(u8, repeat_threshold="3")
    with pytest.raises(ValueError):                                                  # frames of one row, as field_scores refuses them
        savsr_amd.field_stats(torch.zeros(5, 1, 6, 3, dtype=torch.uint8))
    net = SAVSR().eval()
    with pytest.raises(ValueError, match="scan = 'detect' together with fields = 'tff'"):
        net.upscale_video(u8, scan="detect", fields="tff")
    with pytest.raises(ValueError, match="scan = 'detect' together with pulldown = 'bff'"):
        net.upscale_video(u8, scan="detect", pulldown="bff")
    with pytest.raises(ValueError, match="scan = 'detect' with pulldown_cycle = 4"):
        net.upscale_video(u8, scan="detect", pulldown_cycle=4)
    for bad in ("auto", "tff", "progressive", True, 1):
        with pytest.raises(ValueError, match="scan = .*: None or 'detect'"):
            net.upscale_video(u8, scan=bad)
        with pytest.raises(ValueError, match="scan = .*: None or 'detect'"):
            VideoUpscaler(net, 2, scan=bad)
    with pytest.raises(ValueError, match="scan = 'detect' in VideoUpscaler: the decision needs the video.*detect_scan.*fields= or pulldown="):
        VideoUpscaler(net, 2, scan="detect")
    assert VideoUpscaler(net, 2, scan=None)._split is None
    with pytest.raises(ValueError, match="fields = 'auto'"):                         # stays refused
        net.upscale_video(u8, fields="auto")
    assert FIELD_ORDERS == ("tff", "bff") and FIELD_FLAGS == ("progressive", "auto", "tff", "bff")


def test_cli_arguments(tmp_path, capsys):
    from savsr_amd.upscale import parse_args
    base = ["-o", str(tmp_path / "out"), "--scale", "2", "--checkpoint", "net.pth"]
    a = parse_args(["-i", "in.y4m"] + base)
    assert a.scan is None and a.scan_out is None
    a = parse_args(["-i", "in.y4m", "--scan", "detect", "--scan-out", "v.json"] + base)
    assert a.scan == "detect" and a.scan_out == "v.json" and a.fields is None and a.pulldown is None
    a = parse_args(["-i", str(tmp_path), "--scan", "detect", "--crop", "auto", "--cuts", "auto"] + base)          # a PNG folder has no tag: no refusal
    assert a.scan == "detect" and a.crop == "auto"
    for extra, words in ((["-i", "-", "--scan", "detect"], "stdin does not allow: give --fields tff / bff / progressive or --pulldown tff / bff"),
                         (["-i", "in.y4m", "--scan", "detect", "--fields", "tff"], "--scan detect together with --fields tff"),
                         (["-i", "in.y4m", "--scan", "detect", "--fields", "auto"], "--scan detect together with --fields auto"),
                         (["-i", "in.y4m", "--scan", "detect", "--pulldown", "bff"], "--scan detect together with --pulldown bff"),
                         (["-i", "in.y4m", "--scan", "detect", "--pulldown-cycle", "4"], "--pulldown-cycle goes with --pulldown"),
                         (["-i", "in.y4m", "--scan-out", "v.json"], "--scan-out goes with --scan detect"),
                         (["-i", "in.y4m", "--scan", "auto"], "invalid choice")):
        with pytest.raises(SystemExit):
            parse_args(extra + base)
        assert words in capsys.readouterr().err, extra
