"""Chroma siting without a GPU: the siting= half of savsr_amd/yuv.py (the restatement savsr_video_gather_yuvs / savsr_video_quantize_yuvs
are tested against, tests/test_gpu_yuv_siting.py) pinned by ramps (the positions), by the clamped-tap formulas written out per pixel (the
edges), by the paths that must not move (None, "centre" down, 4:4:4) and by the float64 closed form; then the refusals, the Y4M tags and
the CLI's auto / same resolution, on header parsing only."""
import io

import numpy as np
import pytest

from savsr_amd import y4m, yuv
from savsr_amd.upscale import parse_args, resolve_sitings

F32 = np.float32
LAYOUT_SITINGS = [("420", "centre"), ("420", "left"), ("420", "topleft"), ("422", "centre"), ("422", "left")]
EDGE_SIZES = [(1, 1), (1, 2), (2, 1), (3, 5), (4, 6), (5, 4), (2, 2), (7, 6)]


def _frames(n, h, w, depth, chroma, seed=0, over=False):
    ns = yuv.frame_bytes(h, w, 8, chroma)
    s = np.random.RandomState(seed).randint(0, 1 << depth, size=(n, ns))
    if depth == 8:
        return s.astype(np.uint8)
    s = s.astype("<u2")
    if over:
        ch, cw = yuv.chroma_hw(h, w, chroma)
        s[0, 0], s[0, h * w], s[0, h * w + ch * cw] = 1 << depth, 0xffff, (1 << depth) + 5
    return s.view(np.uint8)


def _join(y, u, v, depth):
    n = y.shape[0]
    return np.concatenate([p.astype(np.uint8 if depth == 8 else "<u2").reshape(n, -1) for p in (y, u, v)], 1).view(np.uint8)


def _cosited(siting):
    """(x axis cosited, y axis cosited)"""
    return siting != "centre", siting == "topleft"


# ------------------------------------------------------------------------------------------------------------------- 1, 2: the positions
@pytest.mark.parametrize("chroma,siting", LAYOUT_SITINGS)
def test_a_ramp_in_the_siting_s_positions_reconstructs_to_the_luma_ramp(chroma, siting):
    h, w = 10, 12
    ch, cw = yuv.chroma_hw(h, w, chroma)
    a, b, d = 7, 2, 4                                            # even slopes: the samples a + b (2 c + 0.5) are integers
    cosx, cosy = _cosited(siting)
    px = 2 * np.arange(cw) + (0 if cosx else 0.5)                # where the samples lie, in luma pixels
    py = (2 * np.arange(ch) + (0 if cosy else 0.5)) if chroma == "420" else np.arange(ch)
    plane = (a + b * px[None, :] + d * py[:, None])
    assert np.array_equal(plane, np.round(plane))
    got = yuv.interpolate_chroma(plane[None].astype(np.int64), h, w, chroma, siting)
    assert got.dtype == np.float32 and got.shape == (1, h, w)
    want = a + b * np.arange(w)[None, :] + d * np.arange(h)[:, None]
    x0, x1 = (0, w - 1) if cosx else (1, w - 1)                  # interior: between the first and the last sample of the axis
    y0, y1 = (0, h) if chroma == "422" else ((0, h - 1) if cosy else (1, h - 1))
    assert np.array_equal(got[0, y0:y1, x0:x1], want[y0:y1, x0:x1].astype(np.float32))
    # and the other horizontal siting misses it by b / 2
    other = "left" if siting == "centre" else "centre"
    miss = yuv.interpolate_chroma(plane[None].astype(np.int64), h, w, chroma, other)
    assert np.all(np.abs(miss[0, 2:h - 2, 2:w - 2] - want[2:h - 2, 2:w - 2]) >= b / 2)


@pytest.mark.parametrize("chroma", ["420", "422"])
def test_an_rgb_ramp_filters_down_to_the_siting_s_positions(chroma):
    H, W = 8, 14
    a, b = 3.0, 2.0
    p = np.broadcast_to((a + b * np.arange(W, dtype=F32))[None, None, None, :], (1, 3, H, W)).astype(F32).copy()
    c = np.arange(1, (W + 1) // 2)                               # interior samples
    left = yuv.filter_chroma_rgb(p, chroma, "left")
    centre = yuv.filter_chroma_rgb(p, chroma, "centre")
    assert left.shape == centre.shape == (1, 3) + yuv.chroma_hw(H, W, chroma)
    assert np.array_equal(left[0, 0, :, 1:], np.broadcast_to(a + 2 * b * c, left[0, 0, :, 1:].shape))
    assert np.array_equal(centre[0, 0, :, 1:], np.broadcast_to(a + b * (2 * c + 0.5), centre[0, 0, :, 1:].shape))
    assert np.all(centre[0, :, :, 1:] - left[0, :, :, 1:] == b / 2)
    if chroma == "420":                                          # the same vertically: topleft sits on row 2 cy, left between 2 cy and 2 cy + 1
        q = np.ascontiguousarray(p.transpose(0, 1, 3, 2))        # [1, 3, W, H]: a ramp down the rows
        r = np.arange(1, (W + 1) // 2)
        top, lft = yuv.filter_chroma_rgb(q, "420", "topleft"), yuv.filter_chroma_rgb(q, "420", "left")
        assert np.array_equal(top[0, 0, 1:, 0], a + 2 * b * r) and np.array_equal(lft[0, 0, 1:, 0], a + b * (2 * r + 0.5))


# ----------------------------------------------------------------------------------------------------------------------- 3: the edges
def _interp_by_hand(plane, h, w, chroma, siting):
    """interpolate_chroma one pixel at a time, the table of the module's docstring with every index clamped."""
    ch, cw = plane.shape
    cosx, cosy = _cosited(siting)

    def axis(get, n, p, cos):                                    # numerator over 4 at pixel p of an axis of n samples
        c = p // 2
        if cos:
            return 4 * get(c) if p % 2 == 0 else 2 * get(c) + 2 * get(min(c + 1, n - 1))
        return 3 * get(c) + (get(max(c - 1, 0)) if p % 2 == 0 else get(min(c + 1, n - 1)))
    out = np.empty((h, w), F32)
    for y in range(h):
        for x in range(w):
            if chroma == "422":
                out[y, x] = F32(axis(lambda c: int(plane[y, c]), cw, x, cosx)) * F32(0.25)
            else:
                num = axis(lambda r: axis(lambda c: int(plane[r, c]), cw, x, cosx), ch, y, cosy)
                out[y, x] = F32(num) * F32(0.0625)
    return out


def _filter_by_hand(p, chroma, siting):
    """filter_chroma_rgb of one channel [H, W] for "left" / "topleft", one sample at a time."""
    H, W = p.shape
    ch, cw = yuv.chroma_hw(H, W, chroma)

    def h3(l, c, r):
        return F32(F32(F32(l + r) + F32(c + c)) * F32(0.25))

    def hrow(y, cx):
        return h3(p[y, max(2 * cx - 1, 0)], p[y, 2 * cx], p[y, min(2 * cx + 1, W - 1)])
    out = np.empty((ch, cw), F32)
    for cy in range(ch):
        for cx in range(cw):
            if chroma == "422":
                out[cy, cx] = hrow(cy, cx)
            elif siting == "topleft":
                out[cy, cx] = h3(hrow(max(2 * cy - 1, 0), cx), hrow(2 * cy, cx), hrow(min(2 * cy + 1, H - 1), cx))
            elif 2 * cy + 1 < H:
                out[cy, cx] = F32(F32(hrow(2 * cy, cx) + hrow(2 * cy + 1, cx)) * F32(0.5))
            else:
                out[cy, cx] = hrow(2 * cy, cx)
    return out


@pytest.mark.parametrize("h,w", EDGE_SIZES)
def test_edges_are_the_clamped_tap_formulas(h, w):
    rng = np.random.RandomState(h * 16 + w)
    for chroma, siting in LAYOUT_SITINGS:
        ch, cw = yuv.chroma_hw(h, w, chroma)
        plane = rng.randint(0, 4096, size=(2, ch, cw))
        got = yuv.interpolate_chroma(plane, h, w, chroma, siting)
        for n in range(2):
            assert np.array_equal(got[n], _interp_by_hand(plane[n], h, w, chroma, siting)), (chroma, siting)
        if siting == "centre":
            continue
        p = rng.uniform(0, 1, size=(2, 3, h, w)).astype(F32)
        got = yuv.filter_chroma_rgb(p, chroma, siting)
        for n in range(2):
            for c in range(3):
                assert np.array_equal(got[n, c], _filter_by_hand(p[n, c], chroma, siting)), (chroma, siting)
    # the corner cases spelled out: 1 x 1 is the sample / the pixel itself under every siting
    if (h, w) == (1, 1):
        for chroma, siting in LAYOUT_SITINGS:
            assert yuv.interpolate_chroma(np.array([[[77]]]), 1, 1, chroma, siting)[0, 0, 0] == 77
            assert yuv.filter_chroma_rgb(np.full((1, 3, 1, 1), 0.375, F32), chroma, siting)[0, 0, 0, 0] == F32(0.375)


# --------------------------------------------------------------------------------------------------------------- 4: the unchanged paths
@pytest.mark.parametrize("h,w", [(3, 5), (6, 8), (7, 6)])
def test_none_centre_down_and_444_are_the_code_as_it_stood(h, w):
    x = np.random.RandomState(h + w).uniform(-0.2, 1.2, size=(2, 3, h, w)).astype(F32)
    for depth in (8, 10, 12):
        for chroma in yuv.CHROMAS:
            frames = _frames(2, h, w, depth, chroma, seed=depth, over=True)
            for colour in (yuv.COLOURS if depth == 8 else yuv.COLOURS[:2]):
                down = yuv.rgb_to_i420(x, colour, depth, chroma)
                up = yuv.i420_to_rgb(frames, h, w, colour, depth, chroma)
                assert np.array_equal(yuv.rgb_to_i420(x, colour, depth, chroma, siting=None), down)
                assert np.array_equal(yuv.rgb_to_i420(x, colour, depth, chroma, siting="centre"), down)
                assert np.array_equal(yuv.i420_to_rgb(frames, h, w, colour, depth, chroma, siting=None).view(np.uint32), up.view(np.uint32))
                if chroma == "444":
                    for siting in yuv.SITINGS:
                        assert np.array_equal(yuv.rgb_to_i420(x, colour, depth, chroma, siting=siting), down)
                        assert np.array_equal(yuv.i420_to_rgb(frames, h, w, colour, depth, chroma, siting=siting).view(np.uint32), up.view(np.uint32))
    for a, b in zip(yuv.ycbcr_f32(x, "bt709", "420", "centre"), yuv.ycbcr_f32(x, "bt709", "420")):
        assert np.array_equal(a, b)
    m = np.fmin(np.fmax(x, F32(0)), F32(1))
    assert np.array_equal(yuv.filter_chroma_rgb(m, "422", None), yuv._block_mean(m, "422"))
    # and a cosited output differs from the box where the picture is not flat
    assert not np.array_equal(yuv.rgb_to_i420(x, "bt601", 8, "420", siting="left"), yuv.rgb_to_i420(x, "bt601", 8, "420"))


# ---------------------------------------------------------------------------------------------------------- 5: constant chroma planes
@pytest.mark.parametrize("chroma,siting", LAYOUT_SITINGS)
def test_constant_chroma_planes_give_the_nearest_path_s_rgb(chroma, siting):
    h, w = 7, 6
    ch, cw = yuv.chroma_hw(h, w, chroma)
    rng = np.random.RandomState(5)
    for depth in (8, 10, 12):
        for colour in (yuv.COLOURS if depth == 8 else yuv.COLOURS[:2]):
            n = 16
            y = rng.randint(0, 1 << depth, size=(n, h, w))
            u = np.broadcast_to(rng.randint(0, 1 << depth, size=(n, 1, 1)), (n, ch, cw))
            v = np.broadcast_to(rng.randint(0, 1 << depth, size=(n, 1, 1)), (n, ch, cw))
            frames = _join(y, u, v, depth)
            near = yuv.i420_to_rgb(frames, h, w, colour, depth, chroma)
            got = yuv.i420_to_rgb(frames, h, w, colour, depth, chroma, siting=siting)
            if depth == 8:                                       # the table path and the coefficient path round differently
                assert float(np.abs(got.astype(np.float64) - near.astype(np.float64)).max()) < 1e-6, colour
            else:
                assert np.array_equal(got.view(np.uint32), near.view(np.uint32)), (depth, colour)


# ------------------------------------------------------------------------------------------------------------------ 6: the closed form
def _interp_f64(plane, n_out, axis, off):
    """Linear interpolation in float64 from the positions themselves: sample c lies at 2 c + off; edge samples replicated."""
    nc = plane.shape[axis]
    t = (np.arange(n_out) - off) / 2.0
    c0 = np.floor(t).astype(int)
    f = t - c0
    shape = [1] * plane.ndim
    shape[axis] = n_out
    lo = np.take(plane, np.clip(c0, 0, nc - 1), axis)
    hi = np.take(plane, np.clip(c0 + 1, 0, nc - 1), axis)
    return lo * (1.0 - f).reshape(shape) + hi * f.reshape(shape)


def _closed_form(frames, h, w, colour, depth, chroma, siting):
    t = yuv.matrix(colour)["to_rgb"]
    k = float(1 << (depth - 8))
    top = (1 << depth) - 1
    y, u, v = (np.minimum(p, top).astype(np.float64) for p in yuv.split_planes(frames, h, w, depth, chroma))
    cosx, cosy = _cosited(siting)
    u, v = (_interp_f64(p, w, 2, 0.0 if cosx else 0.5) for p in (u, v))
    if chroma == "420":
        u, v = (_interp_f64(p, h, 1, 0.0 if cosy else 0.5) for p in (u, v))
    o = [x / 255.0 for x in t["offset"]]
    r = y * t["y"] / k + v * t["rv"] / k + o[0]
    g = y * t["y"] / k + u * t["gu"] / k + v * t["gv"] / k + o[1]
    b = y * t["y"] / k + u * t["bu"] / k + o[2]
    return np.clip(np.stack([r, g, b], 1), 0.0, 1.0)


@pytest.mark.parametrize("depth", yuv.DEPTHS)
def test_to_rgb_lies_within_1e_6_of_the_float64_closed_form(depth):
    worst = 0.0
    for chroma, siting in LAYOUT_SITINGS:
        for colour in (yuv.COLOURS if depth == 8 else yuv.COLOURS[:2]):
            for (h, w, over) in ((100, 100, False), (7, 6, True)):         # 10^4 random (y, u, v) per case, and the small odd frame
                frames = _frames(1, h, w, depth, chroma, seed=depth + h, over=over)
                got = yuv.i420_to_rgb(frames, h, w, colour, depth, chroma, siting=siting)
                assert got.dtype == np.float32 and got.shape == (1, 3, h, w)
                err = float(np.abs(got.astype(np.float64) - _closed_form(frames, h, w, colour, depth, chroma, siting)).max())
                worst = max(worst, err)
                assert err < 1e-6, (chroma, siting, colour, h, w, err)
    print(f"depth {depth}: worst |float32 - float64 closed form| = {worst:.3e}")
    assert 5 * 2.5 * 2.0 ** -24 < 1e-6


# ----------------------------------------------------------------------------------------------------------------- 7: refusals, Y4M, CLI
def test_refusals_name_the_rule():
    f = _frames(1, 4, 4, 8, "422")
    x = np.zeros((1, 3, 4, 4), F32)
    with pytest.raises(ValueError, match="siting = 'top': None or one of centre, left, topleft"):
        yuv.i420_to_rgb(_frames(1, 4, 4, 8, "420"), 4, 4, siting="top")
    with pytest.raises(ValueError, match="siting = 1: None or one of centre, left, topleft"):
        yuv.rgb_to_i420(x, siting=1)
    with pytest.raises(ValueError, match="siting = 'topleft' with 4:2:2 chroma: 4:2:2 has no vertical subsampling; its cosited form is 'left'"):
        yuv.i420_to_rgb(f, 4, 4, chroma="422", siting="topleft")
    with pytest.raises(ValueError, match="siting = 'topleft' with 4:2:2 chroma"):
        yuv.rgb_to_i420(x, chroma="422", siting="topleft")
    with pytest.raises(ValueError, match="siting = 'topleft' with 4:2:2 chroma"):
        yuv.interpolate_chroma(np.zeros((1, 4, 2), np.uint8), 4, 4, "422", "topleft")
    with pytest.raises(ValueError, match="siting = None models no siting"):
        yuv.interpolate_chroma(np.zeros((1, 2, 2), np.uint8), 4, 4, "420", None)
    with pytest.raises(ValueError, match="10 and 12 bits are defined for limited range only"):
        yuv.i420_to_rgb(_frames(1, 4, 4, 10, "420"), 4, 4, "bt709-full", 10, siting="left")
    assert yuv.SITINGS == ("centre", "left", "topleft")
    assert [yuv.check_siting(s) for s in (None,) + yuv.SITINGS] == [0, 1, 2, 3]
    # the public arguments, checked on the host before a network or a GPU is needed
    from savsr_amd.video import check_sitings
    assert check_sitings("left", "topleft", "i420", "i420") == (2, 3)
    assert check_sitings(None, "left", "rgb", "i422") == (0, 2)
    with pytest.raises(ValueError, match="siting = 'left' goes with pixel_format = 'i420', 'i422' or 'i444'"):
        check_sitings("left", None, "rgb", "i420")
    with pytest.raises(ValueError, match="out_siting = 'left' goes with out = 'i420', 'i422' or 'i444'"):
        check_sitings(None, "left", "i420", "uint8")
    with pytest.raises(ValueError, match="out_siting = 'topleft' with 4:2:2 chroma"):
        check_sitings(None, "topleft", "i420", "i422")
    with pytest.raises(ValueError, match="siting = 'middle': None or one of"):
        check_sitings("middle", None, "i420", "float")


def _header(ctag, w=6, h=4):
    return f"YUV4MPEG2 W{w} H{h} F25:1 Ip A0:0{'' if ctag is None else ' C' + ctag}\n".encode()


@pytest.mark.parametrize("ctag,siting", [("420jpeg", "centre"), ("420mpeg2", "left"), ("420paldv", "topleft"), ("420", None), (None, None),
                                         ("420p10", None), ("422", None), ("444", None), ("422p12", None)])
def test_y4m_reader_hands_out_the_tag_s_siting(ctag, siting):
    r = y4m.Y4MReader(io.BytesIO(_header(ctag)), high_depth=True, layouts=yuv.CHROMAS)
    assert r.siting == siting
    with pytest.raises(AttributeError):
        r.siting = "left"                                        # read-only
    if ctag in (None, "420", "420jpeg", "420mpeg2", "420paldv"):
        assert y4m.Y4MReader(io.BytesIO(_header(ctag))).siting == siting      # the default constructor reads them as ever
    else:
        with pytest.raises(ValueError, match=f"colour space tag 'C{ctag}' is not supported: 8-bit 4:2:0 only"):
            y4m.Y4MReader(io.BytesIO(_header(ctag)))


def test_y4m_writer_tags_an_8_bit_420_stream_by_its_siting_and_round_trips():
    for siting, tag in ((None, "420jpeg"), ("centre", "420jpeg"), ("left", "420mpeg2"), ("topleft", "420paldv")):
        f = io.BytesIO()
        wr = y4m.Y4MWriter(f, 6, 4, siting=siting)
        assert wr.header == _header(tag)
        frames = _frames(2, 4, 6, 8, "420", seed=1)
        wr.write(frames)
        f.seek(0)
        rd = y4m.Y4MReader(f)
        assert rd.siting == (siting or "centre") and np.array_equal(next(rd.chunks(4)), frames)
    assert y4m.Y4MWriter(io.BytesIO(), 6, 4).header == y4m.Y4MWriter(io.BytesIO(), 6, 4, siting=None).header        # as it was
    for kw, tag in ((dict(depth=10), "420p10"), (dict(chroma="422"), "422"), (dict(chroma="444", depth=12), "444p12")):
        for siting in (None, "left"):
            assert y4m.Y4MWriter(io.BytesIO(), 6, 4, siting=siting, **kw).header == _header(tag)      # no tag for it: unchanged
    with pytest.raises(ValueError, match="y4m: siting = 'mpeg2': None or one of centre, left, topleft"):
        y4m.Y4MWriter(io.BytesIO(), 6, 4, siting="mpeg2")


def test_cli_resolves_auto_and_same_from_the_header():
    base = ["-i", "in.y4m", "-o", "out.y4m", "--scale", "2", "--checkpoint", "net.pth"]
    a = parse_args(base)
    assert (a.siting, a.out_siting) == ("none", "none")                                      # the defaults change nothing
    assert resolve_sitings(a.siting, a.out_siting, "left", "420", "420") == (None, None)
    a = parse_args(base + ["--siting", "auto", "--out-siting", "same"])
    for ctag in ("420jpeg", "420mpeg2", "420paldv", "420", "420p10", "422"):
        r = y4m.Y4MReader(io.BytesIO(_header(ctag)), high_depth=True, layouts=yuv.CHROMAS)
        sin, sout = resolve_sitings(a.siting, a.out_siting, r.siting, r.chroma, r.chroma)
        assert sin == sout == r.siting
        f = io.BytesIO()
        y4m.Y4MWriter(f, 6, 4, depth=r.depth, chroma=r.chroma, siting=sout)
        want = {"420": "420jpeg"}.get(ctag, ctag)                # the writer's tag for what was resolved
        assert f.getvalue() == _header(want)
    assert resolve_sitings("left", "same", None, "422", "420") == ("left", "left")
    assert resolve_sitings("auto", "topleft", "left", "420", "420") == ("left", "topleft")
    assert resolve_sitings("centre", "none", "left", "420", "422") == ("centre", None)
    assert resolve_sitings("auto", "same", "left", "420", "444") == ("left", None)           # 4:4:4 has nothing to resample
    assert resolve_sitings("none", "left", None, None, "420") == (None, "left")              # PNG folder in
    assert resolve_sitings("none", "same", None, None, "420") == (None, None)
    with pytest.raises(ValueError, match="--out-siting = 'topleft' with 4:2:2 chroma"):
        resolve_sitings("auto", "same", "topleft", "420", "422")
    with pytest.raises(ValueError, match="--siting = 'topleft' with 4:2:2 chroma"):
        resolve_sitings("topleft", "none", None, "422", "422")
    for bad in (["--siting", "same"], ["--out-siting", "auto"], ["--siting", "mpeg2"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    with pytest.raises(SystemExit):
        parse_args(["-i", "lr", "-o", "out.y4m", "--scale", "2", "--checkpoint", "n.pth", "--siting", "left"])       # a PNG folder has none
    with pytest.raises(SystemExit):
        parse_args(["-i", "in.y4m", "-o", "sr", "--scale", "2", "--checkpoint", "n.pth", "--out-siting", "left"])
