"""The bwdif deinterlacer's specification (savsr_amd/deinterlace.py `bwdif_matrix`), the method= / rate= arguments of the numpy surface
and `resolve_fields(rate=)`.  No GPU: the kernels are compared with this specification in tests/test_gpu_bwdif.py."""
import numpy as np
import pytest

from savsr_amd import yuv
from savsr_amd.deinterlace import (BRANCHES, BWDIF_BRANCHES, DEINTERLACERS, FIELD_RATES, bwdif_matrix, deinterlace_frames,
                                   deinterlace_frames_counted, deinterlace_matrix, kept_parity, resolve_fields)
from tests.bwdif_cases import ORDERS, SHAPES, inputs, psnr, zone_plate

LF, HF, SP = (4309, 213), (5570, 3801, 1016), (5077, 981)


def _scalar(m, order, depth):
    """The rule of the issue, sample by sample in Python integers (whose >> is the floor, as the rule asks)."""
    N, R, C = m.shape
    top = (1 << depth) - 1
    v = [[[min(int(s), top) for s in row] for row in fr] for fr in m]
    out = np.repeat(m, 2, axis=0)
    for n in range(N):
        cur, prev, nxt = v[n], v[max(n - 1, 0)], v[min(n + 1, N - 1)]
        for f in (0, 1):
            p = kept_parity(order, f)
            p2, n2 = (prev, cur) if f == 0 else (cur, nxt)
            for y in range(1 - p, R, 2):
                up = y + 1 if y == 0 else y - 1
                dn = y - 1 if y == R - 1 else y + 1
                inner = y - 2 >= 0 and y + 2 <= R - 1
                line = y - 4 >= 0 and y + 4 <= R - 1
                for x in range(C):
                    c, e = cur[up][x], cur[dn][x]
                    d = (p2[y][x] + n2[y][x]) >> 1
                    t0 = abs(p2[y][x] - n2[y][x])
                    t1 = (abs(prev[up][x] - c) + abs(prev[dn][x] - e)) >> 1
                    t2 = (abs(nxt[up][x] - c) + abs(nxt[dn][x] - e)) >> 1
                    diff = max(t0 >> 1, t1, t2)
                    if diff == 0:
                        out[2 * n + f, y, x] = d
                        continue
                    wide = diff
                    if inner:
                        b = ((p2[y - 2][x] + n2[y - 2][x]) >> 1) - c
                        g = ((p2[y + 2][x] + n2[y + 2][x]) >> 1) - e
                        mx = max(d - e, d - c, min(b, g))
                        mn = min(d - e, d - c, max(b, g))
                        wide = max(diff, mn, -mx)
                    if line and abs(c - e) > t0:
                        interp = ((HF[0] * (p2[y][x] + n2[y][x]) - HF[1] * (p2[y - 2][x] + n2[y - 2][x] + p2[y + 2][x] + n2[y + 2][x])
                                   + HF[2] * (p2[y - 4][x] + n2[y - 4][x] + p2[y + 4][x] + n2[y + 4][x])) >> 2)
                        interp = (interp + LF[0] * (c + e) - LF[1] * (cur[y - 3][x] + cur[y + 3][x])) >> 13
                    elif line:
                        interp = (SP[0] * (c + e) - SP[1] * (cur[y - 3][x] + cur[y + 3][x])) >> 13
                    else:
                        interp = (c + e) >> 1
                    out[2 * n + f, y, x] = min(max(min(max(interp, d - wide), d + wide), 0), top)
    return out


@pytest.mark.parametrize("depth", [8, 12])
@pytest.mark.parametrize("order", ORDERS)
def test_bwdif_matrix_equals_a_scalar_loop(order, depth):
    top = (1 << depth) - 1
    for r, c in SHAPES:
        for name, v in inputs(r, c, top):
            v = v.astype(np.uint16)
            got, counts = bwdif_matrix(v, order, depth)
            assert got.dtype == v.dtype and got.shape == (2 * v.shape[0], r, c)
            assert np.array_equal(got, _scalar(v, order, depth)), (r, c, name, order, depth)
            assert set(counts) == set(BWDIF_BRANCHES)
            n_interp = sum(len(range(1 - kept_parity(order, f), r, 2)) for f in (0, 1)) * c * v.shape[0]
            assert counts["still"] + counts["line_hf"] + counts["line_sp"] + counts["edge"] == n_interp


@pytest.mark.parametrize("depth", [8, 12])
def test_the_shared_inputs_take_every_branch(depth):
    """A condition on the inputs (it runs on the specification alone): over the shapes, the input set and both orders every branch of
    BWDIF_BRANCHES is taken, or the GPU comparison could not see it."""
    total = dict.fromkeys(BWDIF_BRANCHES, 0)
    for r, c in SHAPES:
        for name, v in inputs(r, c, (1 << depth) - 1):
            for order in ORDERS:
                for k, n in bwdif_matrix(v, order, depth)[1].items():
                    total[k] += n
    assert all(total[k] > 0 for k in BWDIF_BRANCHES), total
    # exactly one `line` row where the shape table says so
    for (r, c), order, y in (((9, 33), "tff", 4), ((10, 32), "bff", 5)):
        f = [f for f in (0, 1) if kept_parity(order, f) == 1 - y % 2][0]
        ys = [yy for yy in range(1 - kept_parity(order, f), r, 2) if yy - 4 >= 0 and yy + 4 <= r - 1]
        assert ys == [y]


@pytest.mark.parametrize("depth", [8, 10, 12])
def test_static_video_comes_back_as_it_is(depth):
    """diff == 0 returns the woven sample: N copies of a picture give 2N copies.  yadif's rule does not (its spatial-interlacing check
    widens a zero clamp), which is why the option exists."""
    top = (1 << depth) - 1
    for r, c in SHAPES:
        pic = np.random.RandomState(r * c + depth).randint(0, top + 1, size=(1, r, c))
        for n in (1, 2, 3):
            for order in ORDERS:
                got = bwdif_matrix(np.repeat(pic, n, 0), order, depth)[0]
                assert np.array_equal(got, np.repeat(pic, 2 * n, 0)), (r, c, n, order)
    if depth == 8:
        pic = np.random.RandomState(3).randint(0, 256, size=(1, 33, 17))
        v = np.repeat(pic, 3, 0)
        assert np.array_equal(bwdif_matrix(v, "tff")[0], np.repeat(pic, 6, 0))
        assert not np.array_equal(deinterlace_matrix(v, "tff")[0], np.repeat(pic, 6, 0))
        u8 = v.astype(np.uint8)[..., None]
        assert np.array_equal(deinterlace_frames(u8, "tff", method="bwdif"), np.repeat(u8[:1], 6, 0))
        assert not np.array_equal(deinterlace_frames(u8, "tff", method="yadif"), np.repeat(u8[:1], 6, 0))


@pytest.mark.parametrize("depth", [10, 12])
def test_kept_rows_are_copied_raw_and_interpolated_samples_stay_in_range(depth):
    top = (1 << depth) - 1
    for r, c in SHAPES:
        v = np.random.RandomState(r + c).randint(0, top + 1, size=(3, r, c)).astype(np.uint16)
        v[:, ::2, ::3] = 60000
        v[1, 1::2, 1::4] = top + 1
        for order in ORDERS:
            got = bwdif_matrix(v, order, depth)[0]
            for n in range(3):
                for f in (0, 1):
                    p = kept_parity(order, f)
                    assert np.array_equal(got[2 * n + f, p::2], v[n, p::2])
                    assert got[2 * n + f, 1 - p::2].max(initial=0) <= top


def test_bwdif_matrix_refuses_what_deinterlace_matrix_refuses():
    for bad, words in ((np.zeros((2, 1, 4), np.uint8), "R = 1"), (np.zeros((2, 4, 0), np.uint8), "R >= 2 and C >= 1"),
                       (np.zeros((0, 4, 4), np.uint8), "no frames"), (np.zeros((2, 4, 4), np.float32), "integers"),
                       (np.zeros((4, 4), np.uint8), "integers")):
        with pytest.raises(ValueError, match=words) as e1:
            bwdif_matrix(bad, "tff")
        with pytest.raises(ValueError) as e2:
            deinterlace_matrix(bad, "tff")
        assert str(e1.value) == str(e2.value)
    with pytest.raises(ValueError, match="depth = 9: 8, 10 or 12"):
        bwdif_matrix(np.zeros((1, 4, 4), np.uint8), "tff", 9)
    with pytest.raises(ValueError, match="order = 'x'"):
        bwdif_matrix(np.zeros((1, 4, 4), np.uint8), "x")


def _frames(kind, rng, n=3):
    if kind == "rgb":
        return rng.randint(0, 256, size=(n, 9, 11, 3), dtype=np.uint8), {}
    fmt, layout, depth, (h, w) = kind
    fb = yuv.frame_bytes(h, w, depth, layout)
    if depth == 8:
        return rng.randint(0, 256, size=(n, fb), dtype=np.uint8), dict(pixel_format=fmt, size=(h, w))
    return (rng.randint(0, 1 << depth, size=(n, fb // 2)).astype("<u2").view(np.uint8).reshape(n, fb),
            dict(pixel_format=fmt, size=(h, w), depth=depth))


KINDS = ["rgb", ("i420", "420", 8, (10, 16)), ("i420", "420", 10, (9, 7)), ("i422", "422", 8, (9, 14)), ("y400", "400", 12, (9, 33))]


def test_frames_with_bwdif_are_the_matrices():
    rng = np.random.RandomState(4)
    v, _ = _frames("rgb", rng)
    n, h, w, c = v.shape
    for order in ORDERS:
        got, counts = deinterlace_frames_counted(v, order, method="bwdif")
        want, cnt = bwdif_matrix(v.reshape(n, h, w * c), order)
        assert np.array_equal(got, want.reshape(2 * n, h, w, c)) and counts == cnt and set(counts) == set(BWDIF_BRANCHES)
    assert set(deinterlace_frames_counted(v, "tff")[1]) == set(BRANCHES)
    for kind in KINDS[1:]:
        frames, kw = _frames(kind, rng)
        fmt, layout, depth, (h, w) = kind
        got = deinterlace_frames(frames, "bff", method="bwdif", **kw)
        planes = [yuv.luma_plane(frames, h, w, depth, layout)] if layout == yuv.MONO else list(yuv.split_planes(frames, h, w, depth, layout))
        want = [bwdif_matrix(p, "bff", depth)[0] for p in planes]
        want = np.concatenate([np.ascontiguousarray(p.astype(np.uint8 if depth == 8 else "<u2")).reshape(6, -1).view(np.uint8) for p in want], 1)
        assert np.array_equal(got, want), kind


@pytest.mark.parametrize("method", DEINTERLACERS)
def test_rate_same_is_every_other_frame(method):
    rng = np.random.RandomState(5)
    for kind in KINDS:
        frames, kw = _frames(kind, rng, 4)
        for order in ORDERS:
            double = deinterlace_frames(frames, order, method=method, rate="double", **kw)
            same = deinterlace_frames(frames, order, method=method, rate="same", **kw)
            assert same.shape[0] == 4 and double.shape[0] == 8 and np.array_equal(same, double[0::2]), (kind, order)


def test_the_defaults_are_the_old_results():
    assert DEINTERLACERS == ("yadif", "bwdif") and FIELD_RATES == ("double", "same")
    rng = np.random.RandomState(6)
    for kind in KINDS:
        frames, kw = _frames(kind, rng)
        for order in ORDERS:
            old = deinterlace_frames(frames, order, **kw)
            assert np.array_equal(old, deinterlace_frames(frames, order, method="yadif", rate="double", **kw))
            if kind == "rgb":
                n, h, w, c = frames.shape
                assert np.array_equal(old, deinterlace_matrix(frames.reshape(n, h, w * c), order, c)[0].reshape(2 * n, h, w, c))
    v, _ = _frames("rgb", rng)
    with pytest.raises(ValueError, match="method = 'w3fdif': one of yadif, bwdif"):
        deinterlace_frames(v, "tff", method="w3fdif")
    with pytest.raises(ValueError, match="rate = 'half': one of double, same"):
        deinterlace_frames(v, "tff", rate="half")


@pytest.mark.parametrize("order", ORDERS)
def test_zone_plate_bwdif_is_closer_to_the_truth_than_yadif(order):
    """A moving zone plate, 64 x 96, 16 field times woven into 8 frames; output frames 2 .. 13 (away from the clamped end frames) against
    the progressive truth.  A comparison with the yadif specification: no absolute figure is asserted."""
    truth, woven = zone_plate(order)
    y = psnr(deinterlace_matrix(woven, order)[0][2:14], truth[2:14])
    b = psnr(bwdif_matrix(woven, order)[0][2:14], truth[2:14])
    print(f"zone plate {order}: yadif {y:.2f} dB, bwdif {b:.2f} dB")
    assert b > y, (order, y, b)


def test_resolve_fields_with_a_rate():
    assert resolve_fields("tff", "t", (25, 1)) == ("tff", "p", (50, 1), None)
    assert resolve_fields("tff", "t", (25, 1), "double") == ("tff", "p", (50, 1), None)
    assert resolve_fields("tff", "t", (25, 1), "same") == ("tff", "p", (25, 1), None)
    assert resolve_fields("auto", "b", (30000, 1001), rate="same") == ("bff", "p", (30000, 1001), None)
    assert resolve_fields("bff", None, (25, 1), "same") == ("bff", "p", (25, 1), None)
    assert resolve_fields("auto", "p", (25, 1), "same") == (None, "p", (25, 1), None)
    assert resolve_fields(None, "t", (25, 1), "same")[:3] == (None, "t", (25, 1))
    with pytest.raises(ValueError, match="--field-rate = 'half'"):
        resolve_fields("tff", "t", (25, 1), "half")


def test_cli_flags_go_with_fields_or_scan_detect(capsys):
    from savsr_amd.upscale import parse_args
    base = ["-i", "in.y4m", "-o", "out.y4m", "--scale", "2", "--checkpoint", "net.pth"]
    a = parse_args(base + ["--fields", "tff"])
    assert (a.deinterlacer, a.field_rate) == ("yadif", "double")
    a = parse_args(base + ["--fields", "auto", "--deinterlacer", "bwdif", "--field-rate", "same"])
    assert (a.deinterlacer, a.field_rate) == ("bwdif", "same")
    a = parse_args(base + ["--scan", "detect", "--deinterlacer", "bwdif"])
    assert (a.deinterlacer, a.field_rate) == ("bwdif", "double")
    for more, words in ((["--deinterlacer", "bwdif"], "--deinterlacer goes with --fields"),
                        (["--field-rate", "same"], "--field-rate goes with --fields"),
                        (["--fields", "progressive", "--field-rate", "same"], "--field-rate goes with --fields"),
                        (["--pulldown", "tff", "--deinterlacer", "bwdif"], "--deinterlacer goes with --fields"),
                        (["--fields", "tff", "--deinterlacer", "w3fdif"], "invalid choice"),
                        (["--fields", "tff", "--field-rate", "half"], "invalid choice")):
        with pytest.raises(SystemExit):
            parse_args(base + more)
        assert words in capsys.readouterr().err, more
