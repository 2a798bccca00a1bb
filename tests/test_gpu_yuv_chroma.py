"""YUV 4:2:2 and 4:4:4 on the GPU: savsr_video_gather_yuvp / savsr_video_quantize_yuvp / savsr_video_pair_sad_yuvp bit for bit against
their numpy restatement (savsr_amd/yuv.py and scenes.py with chroma=, which tests/test_yuv_chroma.py pins) and against the 4:2:0
entries, then pixel_format / out = "i422", "i444" of SAVSR.upscale_video, VideoUpscaler, the self-ensemble, the fp16 mode, cuts="auto"
and the CLI against the composition by hand: yuv.i420_to_rgb -> the float path -> yuv.rgb_to_i420."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

import savsr_amd
from savsr_amd import scenes, y4m, yuv
from savsr_amd.packing import get_hw
from savsr_amd.utils import synth
from tests import scene_cases as SC
from tests.test_yuv_chroma import replicated
from tests.test_yuv_depth import grey_ties
from tests.video_cases import WEIGHT_SEED

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LAYOUTS = ("422", "444")
DEPTHS = (8, 10, 12)
# (h, w, bytes the frames lie off a 16-byte boundary): the three smallest odd shapes (an odd last column, a lone column pair), the vector
# path, more than one workgroup of it (64 x 64: 1 024 units), and a w % 4 == 0 image pushed onto the scalar path by its base pointer
# (18 x 20: 360 units in 4:4:4)
CASES = [(2, 2, 0), (3, 5, 0), (5, 3, 0), (8, 12, 0), (64, 64, 0), (18, 20, 2)]
IDX = [2, 0, 0, 1, 2, 2, 0]                               # repeated and out of order


def _colours(depth):
    return (0, 1, 2, 3) if depth == 8 else (0, 1)         # 10 and 12 bits: the limited-range ids


def _lib():
    from savsr_amd import _lib as L
    return L.load()


def _idx(lst):
    return (C.c_int32 * len(lst))(*lst)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cid(chroma):
    return yuv.CHROMAS.index(chroma)


@pytest.fixture(scope="module")
def net3():
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=WEIGHT_SEED), strict=True)
    return net.to(DEV).eval()


def _frames(n, h, w, depth, chroma, seed=0, over=True):
    """n frames of random samples of the layout; at 10 / 12 bits with `over` the first Y, U and V sample of frame 0 lie above 2^depth - 1."""
    ns = yuv.frame_bytes(h, w, 8, chroma)
    s = np.random.RandomState(seed).randint(0, 1 << depth, size=(n, ns))
    if depth == 8:
        return s.astype(np.uint8)
    s = s.astype("<u2")
    if over:
        ch, cw = yuv.chroma_hw(h, w, chroma)
        s[0, 0], s[0, h * w], s[0, h * w + ch * cw] = 1 << depth, 0xffff, (1 << depth) + 5
    return s.view(np.uint8)


def _gather(frames, h, w, idx, colour, depth, chroma, boff=0, expect=0, entry=None):
    """The entry with the frames boff bytes off an allocation's start; the output buffer is poisoned: everything is written, nothing beyond.
    entry: another gather entry to call in its place (the 4:2:0 ones, for the comparison at chroma = 0)."""
    lib = _lib()
    n, fb = frames.shape
    raw = torch.zeros(n * fb + 16, dtype=torch.uint8, device=DEV)
    raw[boff:boff + n * fb] = torch.from_numpy(frames.reshape(-1)).to(DEV)
    total = len(idx) * 3 * h * w
    out = torch.full((total + 64,), float("nan"), device=DEV)
    assert raw.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    if entry is None:
        rc = lib.savsr_video_gather_yuvp(raw.data_ptr() + boff, n, h, w, _idx(idx), len(idx), colour, depth, _cid(chroma), out.data_ptr(), _stream())
    else:
        rc = entry(raw.data_ptr() + boff, n, h, w, _idx(idx), len(idx), out.data_ptr(), _stream())
    torch.cuda.synchronize()
    if expect:
        assert rc == expect and bool(torch.isnan(out).all())          # refused: nothing was launched
        return lib.savsr_last_error()
    assert rc == 0, lib.savsr_last_error()
    assert bool(torch.isnan(out[total:]).all())
    return out[:total].cpu().numpy().reshape(len(idx), 3, h, w)


def _quantize(x, colour, depth, chroma, boff=0, expect=0, entry=None):
    lib = _lib()
    n, _, H, W = x.shape
    fb = yuv.frame_bytes(H, W, depth, chroma if isinstance(chroma, str) else "420")
    src = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    out = torch.full((n * fb + 64 + boff,), 7, dtype=torch.uint8, device=DEV)
    assert src.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    if entry is None:
        cid = _cid(chroma) if isinstance(chroma, str) else chroma
        rc = lib.savsr_video_quantize_yuvp(src.data_ptr(), n, H, W, colour, depth, cid, out.data_ptr() + boff, _stream())
    else:
        rc = entry(src.data_ptr(), n, H, W, out.data_ptr() + boff, _stream())
    torch.cuda.synchronize()
    if expect:
        assert rc == expect and bool((out == 7).all())
        return lib.savsr_last_error()
    assert rc == 0, lib.savsr_last_error()
    assert bool((out[:boff] == 7).all()) and bool((out[boff + n * fb:] == 7).all())
    return out[boff:boff + n * fb].cpu().numpy().reshape(n, fb)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rgb_in(H, W):
    x = np.random.RandomState(H * 3 + W).uniform(-0.25, 1.25, size=(2, 3, H, W)).astype(np.float32)      # below 0 and above 1 included
    x[0, :, 0, 0] = (-3.0, 0.5, 9.0)
    x[1, :, H - 1, W - 1] = (np.nan, 0.25, np.inf)
    x[1, 1, 0, 0] = np.nan
    return x


# --------------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("chroma", LAYOUTS)
@pytest.mark.parametrize("h,w,boff", CASES)
def test_gather_bitwise(h, w, boff, chroma):
    for depth in DEPTHS:
        frames = _frames(3, h, w, depth, chroma, seed=h + w + depth)
        for colour in _colours(depth):
            ref = yuv.i420_to_rgb(frames, h, w, yuv.COLOURS[colour], depth, chroma)
            got = _gather(frames, h, w, IDX, colour, depth, chroma, boff)
            assert np.array_equal(_bits(got), _bits(ref[IDX])), (depth, colour)


@pytest.mark.parametrize("chroma", LAYOUTS)
@pytest.mark.parametrize("H,W,boff", CASES)
def test_quantize_bitwise(H, W, boff, chroma):
    x = _rgb_in(H, W)
    for depth in DEPTHS:
        for colour in _colours(depth):
            ref = yuv.rgb_to_i420(x, yuv.COLOURS[colour], depth, chroma)
            assert np.array_equal(_quantize(x, colour, depth, chroma, boff), ref), (depth, colour)


@pytest.mark.parametrize("h,w,boff", CASES)
def test_chroma_0_gives_the_bytes_of_the_existing_entries(h, w, boff):
    lib = _lib()
    x = _rgb_in(h, w)
    for depth in DEPTHS:
        frames = _frames(3, h, w, depth, "420", seed=h * w + depth)
        for colour in _colours(depth):
            if depth == 8:
                old_g = lambda f, n, hh, ww, ix, ni, o, st: lib.savsr_video_gather_yuv420(f, n, hh, ww, ix, ni, colour, o, st)      # noqa: E731
                old_q = lambda i, n, hh, ww, o, st: lib.savsr_video_quantize_yuv420(i, n, hh, ww, colour, o, st)                    # noqa: E731
            else:
                old_g = lambda f, n, hh, ww, ix, ni, o, st: lib.savsr_video_gather_yuv420_16(f, n, hh, ww, ix, ni, colour, depth, o, st)      # noqa: E731
                old_q = lambda i, n, hh, ww, o, st: lib.savsr_video_quantize_yuv420_16(i, n, hh, ww, colour, depth, o, st)                    # noqa: E731
            new = _gather(frames, h, w, IDX, colour, depth, "420", boff)
            assert np.array_equal(_bits(new), _bits(_gather(frames, h, w, IDX, colour, depth, "420", boff, entry=old_g))), (depth, colour)
            assert np.array_equal(_bits(new), _bits(yuv.i420_to_rgb(frames, h, w, yuv.COLOURS[colour], depth)[IDX]))
            assert np.array_equal(_quantize(x, colour, depth, "420", boff), _quantize(x, colour, depth, "420", boff, entry=old_q)), (depth, colour)


@pytest.mark.parametrize("h,w,boff", [(3, 5, 0), (8, 12, 0), (18, 20, 2)])
def test_replicated_chroma_gives_the_420_kernels_rgb_and_luma_is_shared(h, w, boff):
    x = _rgb_in(h, w)
    for depth in DEPTHS:
        f420 = _frames(3, h, w, depth, "420", seed=h + depth, over=False)
        ref = _gather(f420, h, w, IDX, 1, depth, "420", boff)              # the existing kernels, through chroma = 0
        y420 = yuv.split_planes(_quantize(x, 1, depth, "420", boff), h, w, depth)[0]
        for chroma in LAYOUTS:
            got = _gather(replicated(f420, h, w, depth, chroma), h, w, IDX, 1, depth, chroma, boff)
            assert np.array_equal(_bits(got), _bits(ref)), (depth, chroma)
            assert np.array_equal(yuv.split_planes(_quantize(x, 1, depth, chroma, boff), h, w, depth, chroma)[0], y420), (depth, chroma)


@pytest.mark.parametrize("chroma", LAYOUTS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_quantize_exact_ties_round_half_to_even(depth, chroma):
    ties = grey_ties("bt601", depth)
    ns = sorted(ties)[:256]
    assert len(ns) >= (40 if depth == 8 else 100) and any(n % 2 for n in ns) and any(n % 2 == 0 for n in ns)
    row = np.array([ties[n] for n in ns], np.float32)
    for W in (len(ns) // 4 * 4, len(ns) // 2 * 2 - 1):    # the vector and the scalar variant
        img = np.broadcast_to(row[None, None, None, :W], (1, 3, 4, W)).copy()
        ref = yuv.rgb_to_i420(img, "bt601", depth, chroma)
        want = np.array([n + n % 2 for n in ns[:W]])
        assert np.array_equal(yuv.split_planes(ref, 4, W, depth, chroma)[0][0, 0], want)      # half to even
        assert np.array_equal(_quantize(img, 0, depth, chroma), ref)


def _sad(frames, h, w, depth, chroma, boff=0):
    lib = _lib()
    n, fb = frames.shape
    raw = torch.zeros(n * fb + 16, dtype=torch.uint8, device=DEV)
    raw[boff:boff + n * fb] = torch.from_numpy(frames.reshape(-1)).to(DEV)
    sad = torch.full((n - 1 + 2,), -1, dtype=torch.int64, device=DEV)
    rc = lib.savsr_video_pair_sad_yuvp(raw.data_ptr() + boff, n, h, w, depth, _cid(chroma), sad.data_ptr(), _stream())
    assert rc == 0, lib.savsr_last_error()
    torch.cuda.synchronize()
    assert sad[n - 1:].tolist() == [-1, -1]
    return sad[:n - 1].cpu().numpy()


@pytest.mark.parametrize("h,w,boff", CASES + [(5, 4, 0)])
def test_pair_sad_equals_the_spec_on_the_y_planes(h, w, boff):
    for depth in (8, 10):
        for chroma in ("420",) + LAYOUTS:
            frames = _frames(4, h, w, depth, chroma, seed=h * w + depth)
            y = yuv.split_planes(frames, h, w, depth, chroma)[0]
            y420 = np.concatenate([y.reshape(4, -1), np.zeros((4, yuv.frame_bytes(h, w, 8) - h * w), y.dtype)], 1)
            ref = scenes.pair_sad(y420 if depth == 8 else y420.astype("<u2").view(np.uint8), "i420", (h, w), depth)      # the Y planes alone
            assert np.array_equal(ref, scenes.pair_sad(frames, "i" + chroma, (h, w), depth))
            assert np.array_equal(_sad(frames, h, w, depth, chroma, boff), ref), (depth, chroma)


def test_bad_arguments_are_refused_without_a_launch():
    lib = _lib()
    h, w = 8, 12
    x = np.zeros((1, 3, h, w), np.float32)
    f10, f8 = _frames(2, h, w, 10, "422"), _frames(2, h, w, 8, "444")
    assert b"video_quantize_yuvp: chroma 3 (0 = 4:2:0, 1 = 4:2:2, 2 = 4:4:4)" in _quantize(x, 0, 8, 3, expect=-1)
    assert b"video_quantize_yuvp: chroma -1" in _quantize(x, 0, 10, -1, expect=-1)
    assert b"video_gather_yuvp: depth 9 (8, 10 or 12)" in _gather(f8, h, w, [0], 0, 9, "444", expect=-1)
    assert b"video_quantize_yuvp: depth 14 (8, 10 or 12)" in _quantize(x, 0, 14, "422", expect=-1)
    assert b"video_gather_yuvp: frames must be 2-byte aligned" in _gather(f10, h, w, [0], 0, 10, "422", boff=1, expect=-1)
    assert b"video_quantize_yuvp: out must be 2-byte aligned" in _quantize(x, 0, 12, "444", boff=3, expect=-1)
    assert b"video_gather_yuvp: colour 2 (0 .. 1: 10 and 12 bits are defined for limited range only)" in _gather(f10, h, w, [0], 2, 10, "422", expect=-1)
    assert b"video_quantize_yuvp: colour 3 (0 .. 1: 10 and 12 bits are defined for limited range only)" in _quantize(x, 3, 10, "444", expect=-1)
    assert b"video_gather_yuvp: colour 4 (0 .. 3)" in _gather(f8, h, w, [0], 4, 8, "444", expect=-1)
    assert b"video_gather_yuvp: slot 1 names frame 2 of 2" in _gather(f8, h, w, [0, 2], 0, 8, "444", expect=-1)
    assert b"video_gather_yuvp: 65 slots (1 .. 64)" in _gather(f10, h, w, [0] * 65, 0, 10, "422", expect=-1)
    out = torch.full((16,), float("nan"), device=DEV)
    assert lib.savsr_video_gather_yuvp(None, 2, h, w, _idx([0]), 1, 0, 8, 1, out.data_ptr(), _stream()) == -1
    assert b"video_gather_yuvp: null pointer" in lib.savsr_last_error()
    assert lib.savsr_video_quantize_yuvp(out.data_ptr(), 1, 2, 2, 0, 8, 2, None, _stream()) == -1
    assert b"video_quantize_yuvp: null pointer" in lib.savsr_last_error()
    fd = torch.zeros(2 * yuv.frame_bytes(h, w, 10, "444") + 16, dtype=torch.uint8, device=DEV)
    sad = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    for args, msg in (((fd.data_ptr() + 1, 2, h, w, 10, 2), b"video_pair_sad_yuvp: frames must be 2-byte aligned"),
                      ((fd.data_ptr(), 2, h, w, 10, 3), b"video_pair_sad_yuvp: chroma 0 (4:2:0), 1 (4:2:2) or 2 (4:4:4)"),
                      ((fd.data_ptr(), 2, h, w, 9, 1), b"video_pair_sad_yuvp: depth 8, 10 or 12")):
        assert lib.savsr_video_pair_sad_yuvp(*args, sad.data_ptr(), _stream()) == -1
        assert msg in lib.savsr_last_error()
    torch.cuda.synchronize()
    assert sad.tolist() == [-1] * 4 and bool(torch.isnan(out).all())
    # the public path names the layout and the pointer
    fb = yuv.frame_bytes(h, w, 10, "422")
    odd = torch.zeros(9 * fb + 1, dtype=torch.uint8, device=DEV)[1:].view(9, fb)
    with pytest.raises(ValueError, match="10-bit I422 frames hold 16-bit samples: the base pointer 0x[0-9a-f]+ is not 2-byte aligned"):
        savsr_amd.pair_sad(odd, "i422", (h, w), depth=10)


def test_kernels_are_capturable_on_a_single_stream():
    """No allocation, no host synchronisation: the three entries record into a hipGraph and replay."""
    lib = _lib()
    h, w = 9, 14
    frames = _frames(3, h, w, 10, "422", seed=1)
    fd = torch.from_numpy(frames).to(DEV)
    rgb = torch.zeros(2, 3, h, w, device=DEV)
    back = torch.zeros(2, yuv.frame_bytes(h, w, 8, "444"), dtype=torch.uint8, device=DEV)
    sad = torch.zeros(2, dtype=torch.int64, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            st = torch.cuda.current_stream().cuda_stream
            assert lib.savsr_video_gather_yuvp(fd.data_ptr(), 3, h, w, _idx([2, 0]), 2, 1, 10, 1, rgb.data_ptr(), st) == 0
            assert lib.savsr_video_quantize_yuvp(rgb.data_ptr(), 2, h, w, 2, 8, 2, back.data_ptr(), st) == 0
            assert lib.savsr_video_pair_sad_yuvp(fd.data_ptr(), 3, h, w, 10, 1, sad.data_ptr(), st) == 0
        g.replay()
    s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    ref = yuv.i420_to_rgb(frames[[2, 0]], h, w, "bt709", 10, "422")
    assert np.array_equal(_bits(rgb.cpu().numpy()), _bits(ref))
    assert np.array_equal(back.cpu().numpy(), yuv.rgb_to_i420(ref, "bt601-full", 8, "444"))
    assert np.array_equal(sad.cpu().numpy(), scenes.pair_sad(frames, "i422", (h, w), 10))


# ------------------------------------------------------------------------------------------------------------ the public interface
N, LR, SC_ = 9, (8, 10), (2.5, 3.0)


def _video(depth, chroma, seed=0):
    return _frames(N, LR[0], LR[1], depth, chroma, seed=seed, over=False)


def _by_hand(net, frames, depth, chroma, out_depth, out_chroma, colour="bt601", out_colour=None):
    """yuv.i420_to_rgb -> upscale_video on the float frames -> yuv.rgb_to_i420, the two conversions in numpy."""
    rgb = torch.from_numpy(yuv.i420_to_rgb(frames, LR[0], LR[1], colour, depth, chroma)).to(DEV)
    sr = net.upscale_video(rgb, scale=SC_, out="float")
    return sr, yuv.rgb_to_i420(sr.cpu().numpy(), out_colour or colour, out_depth, out_chroma)


def test_upscale_video_422_in_444_out_equals_the_composition_by_hand(net3):
    h, w = LR
    H, W = get_hw(h, w, SC_)
    f = _video(10, "422", seed=1)
    kw = dict(scale=SC_, pixel_format="i422", size=LR, depth=10)
    sr, want = _by_hand(net3, f, 10, "422", 10, "444")
    got = net3.upscale_video(torch.from_numpy(f), out="i444", out_depth=10, **kw)
    assert got.dtype == torch.uint8 and got.is_cuda and got.shape == (N, yuv.frame_bytes(H, W, 10, "444")) == (N, 6 * H * W)
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(net3.upscale_video(torch.from_numpy(f).to(DEV), out="i444", **kw), got)          # out_depth = None: the input's
    assert torch.equal(net3.upscale_video(torch.from_numpy(f), **kw), sr)                                # float out
    # the sides are independent: 4:2:0 in, 4:4:4 out; RGB in, 4:2:2 out; 4:4:4 in with another colour space, 4:2:0 out
    f8 = _video(8, "420", seed=2)
    got = net3.upscale_video(torch.from_numpy(f8), scale=SC_, pixel_format="i420", size=LR, out="i444")
    assert np.array_equal(got.cpu().numpy(), _by_hand(net3, f8, 8, "420", 8, "444")[1])
    u8 = torch.from_numpy(np.random.RandomState(4).randint(0, 256, size=(N, h, w, 3), dtype=np.uint8))
    got = net3.upscale_video(u8, scale=SC_, out="i422", out_depth=12, out_colour="bt709")
    want = yuv.rgb_to_i420(net3.upscale_video(u8, scale=SC_).cpu().numpy(), "bt709", 12, "422")
    assert got.shape == (N, yuv.frame_bytes(H, W, 12, "422")) and np.array_equal(got.cpu().numpy(), want)
    f4 = _video(8, "444", seed=3)
    got = net3.upscale_video(torch.from_numpy(f4), scale=SC_, pixel_format="i444", size=LR, colour="bt709-full", out="i420", out_colour="bt601")
    assert np.array_equal(got.cpu().numpy(), _by_hand(net3, f4, 8, "444", 8, "420", "bt709-full", "bt601")[1])


def test_video_upscaler_any_chunking_is_bitwise(net3):
    from savsr_amd import VideoUpscaler
    H, W = get_hw(*LR, SC_)
    frames = torch.from_numpy(_video(10, "422", seed=6))
    kw = dict(out="i444", pixel_format="i422", size=LR, depth=10, out_depth=10)
    whole = net3.upscale_video(frames, scale=SC_, **kw)
    for chunk in (1, 4, 9):
        up = VideoUpscaler(net3, SC_, **kw)
        parts = [up.push(frames[a:a + chunk] if chunk == 1 else frames[a:a + chunk].to(DEV)) for a in range(0, N, chunk)] + [up.finish()]
        assert all(p.dtype == torch.uint8 and p.shape[1] == yuv.frame_bytes(H, W, 10, "444") for p in parts)
        assert torch.equal(torch.cat(parts, 0), whole), chunk


def test_self_ensemble_and_fp16_are_the_composition(net3):
    f = _video(10, "422", seed=5)
    kw = dict(scale=SC_, pixel_format="i422", size=LR, depth=10, out="i444")
    plain = net3.upscale_video(torch.from_numpy(f), **kw)
    net3.set_self_ensemble(True)
    net3.set_precision("fp16")
    try:
        got = net3.upscale_video(torch.from_numpy(f), out_depth=12, **kw)
        want = _by_hand(net3, f, 10, "422", 12, "444")[1]
        both = net3.upscale_video(torch.from_numpy(f), **kw)
    finally:
        net3.set_self_ensemble(False)
        net3.set_precision("fp32")
    assert np.array_equal(got.cpu().numpy(), want) and not torch.equal(both, plain)          # (the switches acted)


def test_auto_cuts_on_444_input_are_the_420_videos(net3):
    from savsr_amd import VideoUpscaler
    v = SC.edited_video()
    h, w = SC.SCENE_HW
    rgb = (v.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2)
    y0, y4 = torch.from_numpy(yuv.rgb_to_i420(rgb)), torch.from_numpy(yuv.rgb_to_i420(rgb, chroma="444"))
    found = savsr_amd.detect_cuts(y0, pixel_format="i420", size=(h, w))
    assert found == SC.SCENE_CUTS
    kw = dict(pixel_format="i444", size=(h, w))
    assert torch.equal(savsr_amd.pair_sad(y4, **kw), savsr_amd.pair_sad(y0, pixel_format="i420", size=(h, w)))
    assert savsr_amd.detect_cuts(y4, **kw) == found == savsr_amd.detect_cuts(y4.to(DEV), **kw)
    whole = net3.upscale_video(y4, scale=2, out="i444", cuts="auto", **kw)
    assert torch.equal(whole, net3.upscale_video(y4, scale=2, out="i444", cuts=found, **kw))
    assert not torch.equal(whole, net3.upscale_video(y4, scale=2, out="i444", **kw))
    up = VideoUpscaler(net3, 2, out="i444", cuts="auto", **kw)
    got = torch.cat([up.push(y4[a:a + 4]) for a in range(0, len(v), 4)] + [up.finish()], 0)
    assert torch.equal(got, whole) and up.cuts == found


# ---------------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_reads_c422p10_and_writes_c444p10_and_out_chroma_420(net3, tmp_path, capsys):
    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    h, w = LR
    sc = (2.0, 3.0)
    H, W = get_hw(h, w, sc)
    ckpt, src = tmp_path / "net.pth", tmp_path / "lr422p10.y4m"
    sio.save_network(net3, str(ckpt))
    frames = _video(10, "422", seed=21)
    with open(src, "wb") as f:
        y4m.Y4MWriter(f, w, h, (30, 1), "p", (1, 1), depth=10, chroma="422").write(frames)
    base = ["-i", str(src), "--scale", "2", "3", "--checkpoint", str(ckpt), "--chunk", "4"]
    for flag, out_chroma in ((["--out-chroma", "444"], "444"), (["--out-chroma", "420"], "420"), ([], "422")):
        dst = tmp_path / f"sr{out_chroma}.y4m"
        assert main(base + ["-o", str(dst)] + flag) == 0
        assert f"upscaled {N} frames" in capsys.readouterr().out
        sr = net3.upscale_video(torch.from_numpy(frames), scale=sc, out="i" + out_chroma, pixel_format="i422", size=(h, w), depth=10).cpu().numpy()
        f = io.BytesIO()
        y4m.Y4MWriter(f, W, H, (30, 1), "p", y4m.scaled_aspect((1, 1), (h, w), (H, W)), depth=10, chroma=out_chroma).write(sr)
        data = dst.read_bytes()
        assert data.startswith(b"YUV4MPEG2 W30 H16 F30:1 Ip A2:3 C" + f"{out_chroma}p10".encode() + b"\n")
        assert data == f.getvalue(), out_chroma
