"""Chroma siting on the GPU: savsr_video_gather_yuvs / savsr_video_quantize_yuvs bit for bit against their numpy restatement
(savsr_amd/yuv.py with siting=, which tests/test_yuv_siting.py pins) and, where they must run the existing kernels, against
savsr_video_gather_yuvp / savsr_video_quantize_yuvp; then siting / out_siting of SAVSR.upscale_video, VideoUpscaler, the self-ensemble
and cuts= against the composition by hand: yuv.i420_to_rgb(siting=) -> the float path -> yuv.rgb_to_i420(siting=)."""
import numpy as np
import pytest
import torch

from savsr_amd import yuv
from savsr_amd.packing import get_hw
from tests.test_gpu_yuv_chroma import DEV, _bits, _cid, _idx, _lib, _stream, net3  # noqa: F401  (net3: the small-network fixture)

pytestmark = pytest.mark.gpu
DEPTHS = (8, 10, 12)
SITINGS_OF = {"420": ("centre", "left", "topleft"), "422": ("centre", "left")}
# (h, w, samples the frames lie off their alignment).  Vector path: 6 x 16 (the first and the last 4-pixel group of a row in one warp),
# 36 x 64 (288 / 576 units: a neighbour across a workgroup boundary and across a row end), 1 x 4 and 2 x 4 (no row above or below).
# Scalar path: the odd sizes, 30 x 35 (270 / 540 units, a workgroup boundary) and 6 x 16 pushed onto it by its base pointer.
CASES = [(6, 16, 0), (36, 64, 0), (1, 4, 0), (2, 4, 0), (1, 1, 0), (2, 2, 0), (5, 3, 0), (7, 6, 0), (30, 35, 0), (6, 16, 1)]
IDX = [2, 0, 0, 1, 2, 2, 0]                               # repeated and out of order
E_ARG = -1


def _colours(depth):
    return (0, 1, 2, 3) if depth == 8 else (0, 1)         # 10 and 12 bits: the limited-range ids


def _sid(siting):
    return yuv.check_siting(siting) if siting is None or isinstance(siting, str) else siting


def _frames(n, h, w, depth, chroma, seed=0):
    """n frames of random codes over the whole sample range: at 10 / 12 bits every 16-bit word, codes above 2^depth - 1 included."""
    ns = yuv.frame_bytes(h, w, 8, chroma)
    rng = np.random.RandomState(seed)
    if depth == 8:
        return rng.randint(0, 256, size=(n, ns)).astype(np.uint8)
    s = rng.randint(0, 1 << depth, size=(n, ns))
    over = rng.uniform(size=(n, ns)) < 0.15
    s[over] = rng.randint(1 << depth, 1 << 16, size=int(over.sum()))
    s[0, 0] = 0xffff
    return s.astype("<u2").view(np.uint8)


def _rgb_in(H, W, seed=0):
    rng = np.random.RandomState(H * 3 + W + seed)
    x = rng.uniform(-0.2, 1.2, size=(2, 3, H, W)).astype(np.float32)
    nan = rng.uniform(size=x.shape) < 0.03
    x[nan] = np.nan
    x[1, 1, 0, 0] = np.nan
    x[0, 2, H - 1, W - 1] = np.inf
    return x


def _gather(frames, h, w, idx, colour, depth, chroma, siting, boff=0, expect=0, old=False):
    """savsr_video_gather_yuvs (old: savsr_video_gather_yuvp) with the frames boff bytes off an allocation's start; the output buffer is
    poisoned: everything is written, nothing beyond."""
    lib = _lib()
    n, fb = frames.shape
    raw = torch.zeros(n * fb + 16, dtype=torch.uint8, device=DEV)
    raw[boff:boff + n * fb] = torch.from_numpy(frames.reshape(-1)).to(DEV)
    total = len(idx) * 3 * h * w
    out = torch.full((total + 64,), float("nan"), device=DEV)
    assert raw.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    cid = _cid(chroma) if isinstance(chroma, str) else chroma
    if old:
        rc = lib.savsr_video_gather_yuvp(raw.data_ptr() + boff, n, h, w, _idx(idx), len(idx), colour, depth, cid, out.data_ptr(), _stream())
    else:
        rc = lib.savsr_video_gather_yuvs(raw.data_ptr() + boff, n, h, w, _idx(idx), len(idx), colour, depth, cid, _sid(siting), out.data_ptr(), _stream())
    torch.cuda.synchronize()
    if expect:
        assert rc == expect and bool(torch.isnan(out).all())          # refused: nothing was launched
        return lib.savsr_last_error()
    assert rc == 0, lib.savsr_last_error()
    assert bool(torch.isnan(out[total:]).all())
    got = out[:total]
    assert not bool(torch.isnan(got).any())
    return got.cpu().numpy().reshape(len(idx), 3, h, w)


def _quantize(x, colour, depth, chroma, siting, boff=0, expect=0, old=False):
    lib = _lib()
    n, _, H, W = x.shape
    fb = yuv.frame_bytes(H, W, depth if depth in DEPTHS else 8, chroma if isinstance(chroma, str) else "420")
    src = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    out = torch.full((n * fb + 64 + boff,), 7, dtype=torch.uint8, device=DEV)
    assert src.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    cid = _cid(chroma) if isinstance(chroma, str) else chroma
    if old:
        rc = lib.savsr_video_quantize_yuvp(src.data_ptr(), n, H, W, colour, depth, cid, out.data_ptr() + boff, _stream())
    else:
        rc = lib.savsr_video_quantize_yuvs(src.data_ptr(), n, H, W, colour, depth, cid, _sid(siting), out.data_ptr() + boff, _stream())
    torch.cuda.synchronize()
    if expect:
        assert rc == expect and bool((out == 7).all())
        return lib.savsr_last_error()
    assert rc == 0, lib.savsr_last_error()
    assert bool((out[:boff] == 7).all()) and bool((out[boff + n * fb:] == 7).all())
    return out[boff:boff + n * fb].cpu().numpy().reshape(n, fb)


def _boff(samples, depth):
    return samples * (1 if depth == 8 else 2)


# --------------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("chroma", ("420", "422"))
@pytest.mark.parametrize("h,w,off", CASES)
def test_gather_bitwise(h, w, off, chroma):
    for depth in DEPTHS:
        frames = _frames(3, h, w, depth, chroma, seed=h + w + depth)
        for siting in SITINGS_OF[chroma]:
            for colour in _colours(depth):
                ref = yuv.i420_to_rgb(frames, h, w, yuv.COLOURS[colour], depth, chroma, siting=siting)
                got = _gather(frames, h, w, IDX, colour, depth, chroma, siting, _boff(off, depth))
                assert np.array_equal(_bits(got), _bits(ref[IDX])), (depth, siting, colour)


@pytest.mark.parametrize("chroma", ("420", "422"))
@pytest.mark.parametrize("H,W,off", CASES)
def test_quantize_bitwise(H, W, off, chroma):
    x = _rgb_in(H, W)
    for depth in DEPTHS:
        for siting in SITINGS_OF[chroma][1:]:              # the cosited ones: the new kernel
            for colour in _colours(depth):
                ref = yuv.rgb_to_i420(x, yuv.COLOURS[colour], depth, chroma, siting=siting)
                assert np.array_equal(_quantize(x, colour, depth, chroma, siting, _boff(off, depth)), ref), (depth, siting, colour)


@pytest.mark.parametrize("h,w,off", [(6, 16, 0), (7, 6, 0), (30, 35, 0), (6, 16, 1)])
def test_siting_0_centre_down_and_444_run_the_existing_entries_bytes(h, w, off):
    x = _rgb_in(h, w, seed=1)
    for depth in DEPTHS:
        b = _boff(off, depth)
        for chroma in yuv.CHROMAS:
            frames = _frames(3, h, w, depth, chroma, seed=h * w + depth)
            for colour in _colours(depth)[::3] + _colours(depth)[1:2]:
                old_g = _gather(frames, h, w, IDX, colour, depth, chroma, None, b, old=True)
                old_q = _quantize(x, colour, depth, chroma, None, b, old=True)
                assert np.array_equal(_bits(_gather(frames, h, w, IDX, colour, depth, chroma, 0, b)), _bits(old_g)), (depth, chroma, colour)
                assert np.array_equal(_quantize(x, colour, depth, chroma, 0, b), old_q), (depth, chroma, colour)
                assert np.array_equal(_quantize(x, colour, depth, chroma, 1, b), old_q), (depth, chroma, colour)          # the box is centre-sited
                if chroma == "444":
                    for sid in (1, 2, 3):
                        assert np.array_equal(_bits(_gather(frames, h, w, IDX, colour, depth, chroma, sid, b)), _bits(old_g)), (depth, sid)
                        assert np.array_equal(_quantize(x, colour, depth, chroma, sid, b), old_q), (depth, sid)


def test_bad_arguments_are_refused_without_a_launch():
    lib = _lib()
    h, w = 8, 12
    x = np.zeros((1, 3, h, w), np.float32)
    f420, f422, f10 = _frames(2, h, w, 8, "420"), _frames(2, h, w, 8, "422"), _frames(2, h, w, 10, "422")
    assert b"video_gather_yuvs: siting 4 (0 = not modelled, 1 = centre, 2 = left, 3 = topleft)" in _gather(f420, h, w, [0], 0, 8, "420", 4, expect=E_ARG)
    assert b"video_gather_yuvs: siting -1 (0 = not modelled" in _gather(f420, h, w, [0], 0, 8, "420", -1, expect=E_ARG)
    assert b"video_quantize_yuvs: siting 4 (0 = not modelled, 1 = centre, 2 = left, 3 = topleft)" in _quantize(x, 0, 8, "420", 4, expect=E_ARG)
    msg = b"siting 3 (topleft) with chroma 1 (4:2:2): 4:2:2 has no vertical subsampling, its cosited form is siting 2 (left)"
    assert b"video_gather_yuvs: " + msg in _gather(f422, h, w, [0], 0, 8, "422", 3, expect=E_ARG)
    assert b"video_quantize_yuvs: " + msg in _quantize(x, 1, 10, "422", 3, expect=E_ARG)
    # what the entries share with savsr_video_gather_yuvp / _quantize_yuvp, under their own name, sited or not
    assert b"video_quantize_yuvs: chroma 3 (0 = 4:2:0, 1 = 4:2:2, 2 = 4:4:4)" in _quantize(x, 0, 8, 3, 2, expect=E_ARG)
    assert b"video_gather_yuvs: depth 9 (8, 10 or 12)" in _gather(f420, h, w, [0], 0, 9, "420", 2, expect=E_ARG)
    assert b"video_gather_yuvs: frames must be 2-byte aligned" in _gather(f10, h, w, [0], 0, 10, "422", 2, boff=1, expect=E_ARG)
    assert b"video_quantize_yuvs: out must be 2-byte aligned" in _quantize(x, 0, 12, "420", 3, boff=3, expect=E_ARG)
    assert b"video_gather_yuvs: colour 2 (0 .. 1: 10 and 12 bits are defined for limited range only)" in _gather(f10, h, w, [0], 2, 10, "422", 1, expect=E_ARG)
    assert b"video_quantize_yuvs: colour 3 (0 .. 1: 10 and 12 bits are defined for limited range only)" in _quantize(x, 3, 10, "420", 2, expect=E_ARG)
    assert b"video_gather_yuvs: colour 4 (0 .. 3)" in _gather(f420, h, w, [0], 4, 8, "420", 1, expect=E_ARG)
    assert b"video_gather_yuvs: slot 1 names frame 2 of 2" in _gather(f420, h, w, [0, 2], 0, 8, "420", 2, expect=E_ARG)
    assert b"video_gather_yuvs: 65 slots (1 .. 64)" in _gather(f420, h, w, [0] * 65, 0, 8, "420", 0, expect=E_ARG)
    out = torch.full((16,), float("nan"), device=DEV)
    assert lib.savsr_video_gather_yuvs(None, 2, h, w, _idx([0]), 1, 0, 8, 0, 2, out.data_ptr(), _stream()) == E_ARG
    assert b"video_gather_yuvs: null pointer" in lib.savsr_last_error()
    assert lib.savsr_video_quantize_yuvs(out.data_ptr(), 1, 2, 2, 0, 8, 0, 3, None, _stream()) == E_ARG
    assert b"video_quantize_yuvs: null pointer" in lib.savsr_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------------------ the public interface
N, LR, SC_ = 9, (8, 10), (2.5, 3.0)


def _video(depth, chroma, seed=0):
    ns = yuv.frame_bytes(LR[0], LR[1], 8, chroma)
    s = np.random.RandomState(seed).randint(0, 1 << depth, size=(N, ns))
    return s.astype(np.uint8) if depth == 8 else s.astype("<u2").view(np.uint8)


def _by_hand(net, frames, depth, chroma, siting, out_depth, out_chroma, out_siting, **kw):
    """yuv.i420_to_rgb -> upscale_video on the float frames -> yuv.rgb_to_i420, the two conversions in numpy."""
    rgb = torch.from_numpy(yuv.i420_to_rgb(frames, LR[0], LR[1], "bt601", depth, chroma, siting=siting)).to(DEV)
    sr = net.upscale_video(rgb, scale=SC_, out="float", **kw)
    return sr, yuv.rgb_to_i420(sr.cpu().numpy(), "bt601", out_depth, out_chroma, siting=out_siting)


def test_upscale_video_left_in_left_out_equals_the_composition_by_hand(net3):  # noqa: F811
    H, W = get_hw(*LR, SC_)
    f = _video(8, "420", seed=1)
    kw = dict(scale=SC_, pixel_format="i420", size=LR)
    sr, want = _by_hand(net3, f, 8, "420", "left", 8, "420", "left")
    got = net3.upscale_video(torch.from_numpy(f), out="i420", siting="left", out_siting="left", **kw)
    assert got.dtype == torch.uint8 and got.is_cuda and got.shape == (N, yuv.frame_bytes(H, W))
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(net3.upscale_video(torch.from_numpy(f), siting="left", **kw), sr)                      # float out
    # the sides are independent, and neither is a default of the other
    plain = net3.upscale_video(torch.from_numpy(f), out="i420", **kw)
    assert np.array_equal(plain.cpu().numpy(), _by_hand(net3, f, 8, "420", None, 8, "420", None)[1])
    one = net3.upscale_video(torch.from_numpy(f), out="i420", siting="topleft", **kw)
    assert np.array_equal(one.cpu().numpy(), _by_hand(net3, f, 8, "420", "topleft", 8, "420", None)[1])
    other = net3.upscale_video(torch.from_numpy(f), out="i420", out_siting="topleft", **kw)
    assert np.array_equal(other.cpu().numpy(), _by_hand(net3, f, 8, "420", None, 8, "420", "topleft")[1])
    assert not torch.equal(plain, got) and not torch.equal(one, plain) and not torch.equal(other, plain)
    # RGB in, a cosited 4:2:0 out
    u8 = torch.from_numpy(np.random.RandomState(4).randint(0, 256, size=(N, LR[0], LR[1], 3), dtype=np.uint8))
    got = net3.upscale_video(u8, scale=SC_, out="i420", out_siting="left")
    assert np.array_equal(got.cpu().numpy(), yuv.rgb_to_i420(net3.upscale_video(u8, scale=SC_).cpu().numpy(), siting="left"))


def test_upscale_video_i422_at_10_bits(net3):  # noqa: F811
    f = _video(10, "422", seed=2)
    got = net3.upscale_video(torch.from_numpy(f), scale=SC_, pixel_format="i422", size=LR, depth=10, out="i422", siting="left", out_siting="left")
    assert np.array_equal(got.cpu().numpy(), _by_hand(net3, f, 10, "422", "left", 10, "422", "left")[1])
    got = net3.upscale_video(torch.from_numpy(f), scale=SC_, pixel_format="i422", size=LR, depth=10, out="i420", out_depth=12, siting="centre",
                             out_siting="topleft")
    assert np.array_equal(got.cpu().numpy(), _by_hand(net3, f, 10, "422", "centre", 12, "420", "topleft")[1])


def test_video_upscaler_any_chunking_is_bitwise(net3):  # noqa: F811
    from savsr_amd import VideoUpscaler
    frames = torch.from_numpy(_video(8, "420", seed=6))
    kw = dict(out="i420", pixel_format="i420", size=LR, siting="left", out_siting="topleft")
    whole = net3.upscale_video(frames, scale=SC_, **kw)
    assert np.array_equal(whole.cpu().numpy(), _by_hand(net3, frames.numpy(), 8, "420", "left", 8, "420", "topleft")[1])
    for chunk in (1, 4):
        up = VideoUpscaler(net3, SC_, **kw)
        parts = [up.push(frames[a:a + chunk] if chunk == 1 else frames[a:a + chunk].to(DEV)) for a in range(0, N, chunk)] + [up.finish()]
        assert torch.equal(torch.cat(parts, 0), whole), chunk


def test_self_ensemble_converts_once_and_quantises_after_the_merge(net3):  # noqa: F811
    f = _video(8, "420", seed=5)
    kw = dict(scale=SC_, pixel_format="i420", size=LR, out="i420", siting="left", out_siting="left")
    plain = net3.upscale_video(torch.from_numpy(f), **kw)
    net3.set_self_ensemble(True)
    try:
        got = net3.upscale_video(torch.from_numpy(f), **kw)
        want = _by_hand(net3, f, 8, "420", "left", 8, "420", "left")[1]
    finally:
        net3.set_self_ensemble(False)
    assert np.array_equal(got.cpu().numpy(), want) and not torch.equal(got, plain)          # (the switch acted)


def test_cuts_compose(net3):  # noqa: F811
    f = _video(8, "420", seed=7)
    kw = dict(scale=SC_, pixel_format="i420", size=LR, out="i420", siting="left", out_siting="left")
    got = net3.upscale_video(torch.from_numpy(f), cuts=[4], **kw)
    want = _by_hand(net3, f, 8, "420", "left", 8, "420", "left", cuts=[4])[1]
    assert np.array_equal(got.cpu().numpy(), want)
    assert not torch.equal(got, net3.upscale_video(torch.from_numpy(f), **kw))
    # pair_sad reads Y only: the detector's scores do not depend on a siting, and cuts="auto" runs with one
    auto = net3.upscale_video(torch.from_numpy(f), cuts="auto", scene_threshold=99.0, **kw)
    assert auto.shape == got.shape


def test_python_refusals(net3):  # noqa: F811
    from savsr_amd import VideoUpscaler
    f = torch.from_numpy(_video(8, "420"))
    f422 = torch.from_numpy(_video(8, "422"))
    rgb = torch.zeros(N, LR[0], LR[1], 3, dtype=torch.uint8)
    kw = dict(scale=SC_, size=LR)
    for make in (lambda **k: net3.upscale_video(k.pop("frames"), **k), lambda **k: VideoUpscaler(net3, **{a: b for a, b in k.items() if a != "frames"})):
        with pytest.raises(ValueError, match="siting = 'mpeg2': None or one of centre, left, topleft"):
            make(frames=f, pixel_format="i420", siting="mpeg2", **kw)
        with pytest.raises(ValueError, match="out_siting = 2: None or one of centre, left, topleft"):
            make(frames=f, pixel_format="i420", out="i420", out_siting=2, **kw)
        with pytest.raises(ValueError, match="siting = 'topleft' with 4:2:2 chroma: 4:2:2 has no vertical subsampling; its cosited form is 'left'"):
            make(frames=f422, pixel_format="i422", siting="topleft", **kw)
        with pytest.raises(ValueError, match="out_siting = 'topleft' with 4:2:2 chroma"):
            make(frames=f, pixel_format="i420", out="i422", out_siting="topleft", **kw)
        with pytest.raises(ValueError, match="siting = 'left' goes with pixel_format = 'i420', 'i422' or 'i444'"):
            make(frames=rgb, scale=SC_, siting="left")
        with pytest.raises(ValueError, match="out_siting = 'left' goes with out = 'i420', 'i422' or 'i444'"):
            make(frames=f, pixel_format="i420", out="uint8", out_siting="left", **kw)
    eng = net3.engine()
    # at the engine's door: what it takes is a VideoSpec, and there is none with an unknown siting or an out_siting without YUV output,
    # through the factory or around it; anything else in its place is refused before anything is enqueued
    import dataclasses
    from savsr_amd.video import video_spec
    good = video_spec(3, pixel_format="i420", size=LR, siting="left")
    with pytest.raises(ValueError, match="siting = 'mpeg2': None or one of centre, left, topleft"):
        eng.forward_video(f.to(DEV), [[0] * 7], SC_, video_spec(3, pixel_format="i420", size=LR, siting="mpeg2"))
    with pytest.raises(ValueError, match="out_siting = 'left' goes with out = 'i420', 'i422' or 'i444'"):
        eng.forward_video(f.to(DEV), [[0] * 7], SC_, video_spec(3, pixel_format="i420", size=LR, out_siting="left"))
    with pytest.raises(ValueError, match="siting = 4: None or one of centre, left, topleft"):
        eng.forward_video(f.to(DEV), [[0] * 7], SC_, dataclasses.replace(good, inp=dataclasses.replace(good.inp, siting=4)))
    with pytest.raises(ValueError, match="out_siting = 'left' goes with out = 'i420', 'i422' or 'i444'"):
        eng.forward_video(f.to(DEV), [[0] * 7], SC_, dataclasses.replace(good, out=dataclasses.replace(good.out, siting="left")))
    for not_a_spec in (dict(pixel_format="i420", size=LR, siting=1), good.inp, 1, True):
        with pytest.raises(ValueError, match="spec must be a savsr_amd.video.VideoSpec"):
            eng.forward_video(f.to(DEV), [[0] * 7], SC_, not_a_spec)
    assert eng.forward_video(f.to(DEV), [[0] * 7], SC_, good).shape == (1, 3) + get_hw(*LR, SC_)          # (and takes the one that is)
