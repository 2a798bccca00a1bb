"""The pulldown removal's specification (savsr_amd/pulldown.py; no GPU): the forward process, the recovery property on vertically coherent
film of both kinds, the documented losses at the other phases, the two host decisions on hand-made lists, the refusals and the CLI's
header decision."""
import io

import numpy as np
import pytest
import torch

from savsr_amd import pulldown as pd
from savsr_amd import y4m, yuv
from savsr_amd.deinterlace import FIELD_ORDERS
from tests.pulldown_cases import FILM_LENGTHS, KINDS, SIZES, gradient, matrix_film, packed_film, planar_film


# ---------------------------------------------------------------------------------------------------------------------- the forward process
@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_telecine_of_four_film_frames_is_aa_bb_bc_cd_dd(order):
    film = packed_film("gradient", 4, 6, 5)
    A, B, C, D = film
    p = FIELD_ORDERS.index(order)

    def woven(first, second):
        f = first.copy()
        f[1 - p::2] = second[1 - p::2]
        return f
    want = np.stack([woven(A, A), woven(B, B), woven(B, C), woven(C, D), woven(D, D)])
    got = pd.telecine(film, order)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(got[0], A) and np.array_equal(got[4], D) and not np.array_equal(got[2], B) and not np.array_equal(got[2], C)
    assert pd.telecine_sources(4) == ([0, 1, 1, 2, 3], [0, 1, 2, 3, 3])
    assert pd.telecine_sources(3) == ([0, 1, 1], [0, 1, 2])                          # 2 + 3 + 2 fields: the trailing unpaired one is dropped
    assert np.array_equal(pd.telecine(film, order, phase=2), want[2:])
    planar = planar_film("bar", 4, 6, 10)
    got = yuv.split_planes(pd.telecine(planar, order, 0, "i420", (6, 10)), 6, 10)          # every plane on its own, with the luma's parity
    for plane, tele in zip(yuv.split_planes(planar, 6, 10), got):
        assert np.array_equal(tele, pd.telecine(plane[..., None], order)[..., 0])


# ---------------------------------------------------------------------------------------------------------------------- the recovery property
def _recovers(film, order, kw, m):
    video = pd.telecine(film, order, 0, **kw)
    n = video.shape[0]
    assert n == m * 5 // 4
    out, info = pd.remove_pulldown_frames(video, order, **kw)
    # the inputs exercise both candidates and every full cycle has exactly one repeated picture
    assert set(info["matches"]) == {-1, 0}
    sad = info["sad"]
    assert sad[0] == -1 and all(int((sad[c0:c0 + 5] == 0).sum()) == 1 for c0 in range(0, n - 4, 5))
    assert info["kept"] == [k for k in range(n) if k % 5 != 2] and info["scores"].shape == (n, 2) and info["scores"].dtype == np.int64
    assert out.dtype == film.dtype and np.array_equal(out, film)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_phase_0_film_is_recovered_exactly(order, kind):
    for h, w in SIZES:
        for m in FILM_LENGTHS:
            _recovers(packed_film(kind, m, h, w), order, {}, m)


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_phase_0_film_is_recovered_exactly_through_planar_i420(order, kind, depth):
    for h, w in SIZES:
        for m in FILM_LENGTHS:
            _recovers(planar_film(kind, m, h, w, depth), order, dict(pixel_format="i420", size=(h, w), depth=depth), m)


# What comes out at the other phases of a 12-frame film (15 video frames, `phase` leading ones dropped), by film index; -1: a combed frame.
# Derived from the rules by hand (the video is AA BB BC CD DD per four film frames; woven frame n keeps its first field):
#   phase 1  woven 1 1 2 3 4 | 5 5 6 7 8 | 9 9 10 11: the partial last cycle keeps its duplicate
#   phase 2  woven X 2 3 4 5 | 5 6 7 8 9 | 9 10 11, X = first field of 1 with the second of 2 (its partner was cut off): the first cycle has
#            no repeated picture, so decimation drops the frame nearest its predecessor, film frame 2 (half of its rows are X's); the
#            partial last cycle keeps its duplicate
#   phase 3  woven X 3 4 5 5 | 6 7 8 9 9 | 10 11, X = first field of 2 with the second of 3
#   phase 4  woven 3 4 5 5 6 | 7 8 9 9 10 | 11
PHASES = {
    1: [1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 10, 11],
    2: [-1, 3, 4, 5, 6, 7, 8, 9, 9, 10, 11],
    3: [-1, 3, 4, 5, 6, 7, 8, 9, 10, 11],
    4: [3, 4, 5, 6, 7, 8, 9, 10, 11],
}
COMBED = {2: (1, 2), 3: (2, 3)}          # phase -> (film frame of the first field, of the second field) of the combed first frame


@pytest.mark.parametrize("phase", sorted(PHASES))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_other_phases_lose_what_is_documented_and_no_more(order, kind, phase):
    film = packed_film(kind, 12, 9, 33)
    assert len({f.tobytes() for f in film}) == 12                                    # the film frames are told apart by their bytes
    out, info = pd.remove_pulldown_frames(pd.telecine(film, order, phase), order)
    names = {f.tobytes(): k for k, f in enumerate(film)}
    if phase in COMBED:
        a, b = COMBED[phase]
        names[pd.weave(film[[b, a]], order, [0, -1])[1].tobytes()] = -1              # (the first field of a with the second field of b)
    got = [names.get(f.tobytes(), None) for f in out]
    assert got == PHASES[phase]
    assert len(info["kept"]) == (15 - phase) - (15 - phase) // 5


# ---------------------------------------------------------------------------------------------------------------------- the rules
def test_field_scores_are_zero_on_monotone_pictures_and_positive_on_combs():
    ramp = np.repeat(np.arange(0, 70, 10, dtype=np.uint8)[None, :, None], 3, 0).repeat(4, 2)          # [3, 7, 4], rows 0, 10, .. 60
    assert not pd.field_scores(ramp, "tff").any() and not pd.field_scores(ramp, "bff").any()
    v = ramp.copy()
    v[1, 1::2] += 25                                                                  # frame 1's odd rows leave their neighbours' interval by 15
    s = pd.field_scores(v, "tff")                                                     # second field: the odd rows 1, 3, 5
    assert s.tolist() == [[0, 0], [0, 3 * 4 * 2 * 15], [3 * 4 * 2 * 15, 0]]
    s = pd.field_scores(v, "bff")                                                     # second field: the even rows 2, 4 between combed odd rows
    assert s[1].tolist() == [2 * 4 * 2 * 15, 2 * 4 * 2 * 15] and s[0].tolist() == [0, 0]
    for r in (1, 2):
        assert not pd.field_scores(np.random.RandomState(r).randint(0, 256, size=(2, r, 5)), "tff").any()
    three = np.random.RandomState(3).randint(0, 256, size=(2, 3, 5))
    assert pd.field_scores(three, "tff").any() and not pd.field_scores(three, "bff").any()          # one scored row for one order only
    hi = (gradient(2, 5, 6).astype(np.uint16) << 2) | 3
    assert np.array_equal(pd.field_scores(hi, "tff", 10), pd.field_scores(gradient(2, 5, 6), "tff"))
    hi[0, 2, 1] = 60000                                                               # above 2^10 - 1: read as 1023 -> 255
    low = gradient(2, 5, 6)
    low[0, 2, 1] = 255
    assert np.array_equal(pd.field_scores(hi, "bff", 10), pd.field_scores(low, "bff"))


def test_matches_from_scores_ties_keep_the_own_field():
    assert pd.matches_from_scores([[0, 0], [1, 2], [2, 1], [5, 5], [0, 1 << 40]]) == [0, -1, 0, 0, -1]
    assert pd.matches_from_scores(np.zeros((0, 2), np.int64)) == []


def test_weave_takes_the_second_field_from_the_predecessor():
    v = np.random.RandomState(4).randint(0, 256, size=(3, 5, 4, 3), dtype=np.uint8)
    for order, p in (("tff", 0), ("bff", 1)):
        out = pd.weave(v, order, [-1, -1, 0])
        assert np.array_equal(out[0], v[0]) and np.array_equal(out[2], v[2])          # n + delta < 0 clamps; delta 0 is the frame itself
        assert np.array_equal(out[1, p::2], v[1, p::2]) and np.array_equal(out[1, 1 - p::2], v[0, 1 - p::2])
    with pytest.raises(ValueError, match="one of -1, 0 per frame"):
        pd.weave(v, "tff", [0, 1, 0])
    with pytest.raises(ValueError, match="one of -1, 0 per frame"):
        pd.weave(v, "tff", [0, 0])


def test_drops_from_sad_on_hand_made_lists():
    assert pd.drops_from_sad([0, 5, 3, 3, 9]) == [2]                                  # sad[0] counts as infinite; ties drop the lowest index
    assert pd.drops_from_sad([-1, 5, 3, 3, 9, 0, 7, 7, 7, 7]) == [2, 5]
    assert pd.drops_from_sad([-1, 5, 3, 3, 9, 4, 4, 4, 4, 4, 0, 0]) == [2, 5]         # a partial tail keeps all its frames
    assert pd.drops_from_sad([-1, 5, 3, 3]) == [] and pd.drops_from_sad([]) == []
    assert pd.drops_from_sad([-1, 9, 1, 2, 3, 0], cycle=2) == [1, 2, 5]               # cycle 2: frame 0 never, then the smaller of each pair
    assert pd.drops_from_sad([-1] + [7] * 23 + [6] + [0] * 24, cycle=25) == [24]
    assert pd.drops_from_sad([3, 2, 3, 3, 3], first=5) == [6]                         # a later cycle on its own: its first entry counts
    assert pd.kept_from_drops(7, [2, 5]) == [0, 1, 3, 4, 6]
    for bad in (1, 26, 0, -5, 5.0, True, "5", None):
        with pytest.raises(ValueError, match="an int in 2 .. 25"):
            pd.drops_from_sad([0] * 10, cycle=bad)
    with pytest.raises(ValueError, match="multiple of cycle"):
        pd.drops_from_sad([0] * 5, first=3)


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    u8 = np.zeros((5, 4, 6, 3), np.uint8)
    with pytest.raises(ValueError, match="float frames have no integer samples"):
        pd.remove_pulldown_frames(np.zeros((5, 3, 4, 6), np.float32), "tff")
    for bad in ("top", "progressive", None, 0):
        with pytest.raises(ValueError, match="one of tff, bff"):
            pd.remove_pulldown_frames(u8, bad)
    with pytest.raises(ValueError, match="cycle = 1: an int in 2 .. 25"):
        pd.remove_pulldown_frames(u8, "tff", cycle=1)
    with pytest.raises(ValueError, match="no frames"):
        pd.remove_pulldown_frames(u8[:0], "tff")
    with pytest.raises(ValueError, match="one row"):
        pd.remove_pulldown_frames(u8[:, :1], "tff")
    with pytest.raises(ValueError, match=r"are \[N, 36\] uint8"):
        pd.remove_pulldown_frames(np.zeros((5, 35), np.uint8), "tff", "i420", (4, 6))
    with pytest.raises(ValueError, match="packed frames are 8-bit"):
        pd.remove_pulldown_frames(u8, "tff", depth=10)
    with pytest.raises(ValueError, match="phase"):
        pd.telecine(u8, "tff", phase=-1)
    out, info = pd.remove_pulldown_frames(u8[:3], "bff")                              # fewer frames than a cycle: all kept
    assert out.shape == (3, 4, 6, 3) and info["kept"] == [0, 1, 2]


def test_the_public_calls_refuse_before_the_gpu_is_needed():
    import savsr_amd
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.video import VideoUpscaler, _check_pulldown
    u8 = torch.zeros(10, 4, 6, 3, dtype=torch.uint8)
    assert _check_pulldown(None, 5, None) is None and _check_pulldown(None, 5, "tff") is None and _check_pulldown("bff", 4, None) == "bff"
    with pytest.raises(ValueError, match="pulldown = 'tff' together with fields = 'tff'"):
        _check_pulldown("tff", 5, "tff")
    with pytest.raises(ValueError, match="pulldown_cycle = 4 goes with pulldown="):
        _check_pulldown(None, 4, None)
    with pytest.raises(ValueError, match="one of tff, bff"):
        savsr_amd.remove_pulldown(u8, "auto")
    with pytest.raises(ValueError, match="float frames have no integer samples"):
        savsr_amd.remove_pulldown(torch.zeros(5, 3, 4, 6), "tff")
    with pytest.raises(ValueError, match="an int in 2 .. 25"):
        savsr_amd.remove_pulldown(u8, "tff", cycle=26)
    with pytest.raises(ValueError, match="float frames have no integer samples"):
        savsr_amd.field_scores(torch.zeros(5, 3, 4, 6), "tff")
    net = SAVSR().eval()
    with pytest.raises(ValueError, match="pulldown = 'auto': one of tff, bff"):
        net.upscale_video(u8, pulldown="auto")
    with pytest.raises(ValueError, match="together with fields = 'bff'"):
        net.upscale_video(u8, pulldown="tff", fields="bff")
    with pytest.raises(ValueError, match="together with fields"):
        VideoUpscaler(net, 2, pulldown="tff", fields="tff")
    with pytest.raises(ValueError, match="pulldown_cycle = 6 goes with pulldown="):
        net.upscale_video(u8, pulldown_cycle=6)
    with pytest.raises(ValueError, match="pulldown_cycle = 1: an int in 2 .. 25"):
        VideoUpscaler(net, 2, pulldown="tff", pulldown_cycle=1)
    with pytest.raises(ValueError, match="float frames have no integer samples"):
        VideoUpscaler(net, 2, pulldown="tff").push(torch.zeros(2, 3, 4, 6))
    with pytest.raises(ValueError, match="too few"):                                 # check_length applies to the film frames: 2 of them, a 7-frame window
        net.upscale_video(u8[:2], pulldown="tff")


# ---------------------------------------------------------------------------------------------------------------------- the CLI's header
def test_resolve_pulldown():
    ntsc = (30000, 1001)
    for flag in (None, "none"):
        for tag in ("p", "t", "b", "m", "?"):
            assert pd.resolve_pulldown(flag, tag, ntsc) == (None, tag, ntsc, None)
        assert pd.resolve_pulldown(flag, None, (25, 1)) == (None, "p", (25, 1), None)
    assert pd.resolve_pulldown("auto", "t", ntsc) == ("tff", "p", (24000, 1001), None)
    assert pd.resolve_pulldown("auto", "b", (30, 1)) == ("bff", "p", (24, 1), None)
    order, tag, fps, note = pd.resolve_pulldown("auto", "p", ntsc)
    assert (order, tag, fps) == (None, "p", ntsc) and "nothing is removed" in note
    assert pd.resolve_pulldown("tff", "t", ntsc, 6)[2] == (25000, 1001) and pd.resolve_pulldown("tff", None, (25, 1), 2)[2] == (25, 2)
    for flag in FIELD_ORDERS:
        for tag in ("p", "t", "b", "m", None):                                       # an explicit order overrides the tag
            assert pd.resolve_pulldown(flag, tag, ntsc) == (flag, "p", (24000, 1001), None)
    with pytest.raises(ValueError, match="Im"):
        pd.resolve_pulldown("auto", "m", ntsc)
    with pytest.raises(ValueError, match="PNG folder"):
        pd.resolve_pulldown("auto", None, ntsc)
    with pytest.raises(ValueError, match="one of none, auto, tff, bff"):
        pd.resolve_pulldown("top", "t", ntsc)
    with pytest.raises(ValueError, match="--pulldown-cycle = 30"):
        pd.resolve_pulldown("tff", "t", ntsc, 30)
    with pytest.raises(ValueError, match="--pulldown-cycle = 4 goes with --pulldown"):
        pd.resolve_pulldown(None, "t", ntsc, 4)


def test_the_y4m_header_round_trip_of_the_film_rate():
    order, tag, fps, _ = pd.resolve_pulldown("auto", "t", (30000, 1001))
    frames = planar_film("gradient", 2, 4, 6)
    f = io.BytesIO()
    y4m.Y4MWriter(f, 6, 4, fps, tag, (1, 1)).write(frames)
    assert b" F24000:1001 Ip " in f.getvalue()[:60]
    f.seek(0)
    r = y4m.Y4MReader(f)
    assert (r.fps, r.interlace, r.width, r.height) == ((24000, 1001), "p", 6, 4)
    assert np.array_equal(np.concatenate(list(r.chunks(4))), frames)


def test_cli_arguments(tmp_path, capsys):
    from savsr_amd.upscale import parse_args
    base = ["-o", str(tmp_path / "out"), "--scale", "2", "--checkpoint", "net.pth"]
    a = parse_args(["-i", "in.y4m"] + base)
    assert a.pulldown is None and a.pulldown_cycle == 5
    a = parse_args(["-i", "in.y4m", "--pulldown", "auto", "--pulldown-cycle", "6"] + base)
    assert a.pulldown == "auto" and a.pulldown_cycle == 6
    assert parse_args(["-i", str(tmp_path), "--pulldown", "bff"] + base).pulldown == "bff"
    assert parse_args(["-i", "in.y4m", "--pulldown", "tff", "--fields", "progressive"] + base).fields == "progressive"
    for extra, words in ((["-i", str(tmp_path), "--pulldown", "auto"], "PNG folder"),
                         (["-i", "in.y4m", "--pulldown", "tff", "--fields", "tff"], "two answers to one question"),
                         (["-i", "in.y4m", "--pulldown", "auto", "--fields", "auto"], "two answers to one question"),
                         (["-i", "in.y4m", "--pulldown-cycle", "4"], "--pulldown-cycle goes with --pulldown"),
                         (["-i", "in.y4m", "--pulldown", "none", "--pulldown-cycle", "4"], "--pulldown-cycle goes with --pulldown"),
                         (["-i", "in.y4m", "--pulldown", "tff", "--pulldown-cycle", "1"], "an int in 2 .. 25"),
                         (["-i", "in.y4m", "--pulldown", "top"], "invalid choice")):
        with pytest.raises(SystemExit):
            parse_args(extra + base)
        assert words in capsys.readouterr().err, extra
