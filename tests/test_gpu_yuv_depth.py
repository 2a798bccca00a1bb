"""10- and 12-bit YUV 4:2:0 on the GPU: savsr_video_gather_yuv420_16 / savsr_video_quantize_yuv420_16 / savsr_video_pair_sad_i420_16 bit
for bit against their numpy restatement (savsr_amd/yuv.py and scenes.py with depth=, which tests/test_yuv_depth.py pins), then depth /
out_depth of SAVSR.upscale_video, VideoUpscaler, the self-ensemble, the fp16 mode, cuts="auto" and the CLI against the composition by
hand: yuv.i420_to_rgb -> the float path -> yuv.rgb_to_i420."""
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
from tests.test_yuv_depth import grey_ties
from tests.video_cases import WEIGHT_SEED

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DEPTHS = (10, 12)
COLOURS = (0, 1)                                          # bt601, bt709: the limited-range ids
# (h, w, bytes the frames lie off a 16-byte boundary): the three smallest odd shapes, the vector path, every 12-bit Y and every 10-bit
# chroma code, and a w % 4 == 0 image pushed onto the 2 x 2 path by its base pointer
CASES = [(2, 2, 0), (3, 5, 0), (5, 3, 0), (8, 12, 0), (64, 64, 0), (18, 20, 2)]
MAX_SLOTS = 64


def _lib():
    from savsr_amd import _lib as L
    return L.load()


def _idx(lst):
    return (C.c_int32 * len(lst))(*lst)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def net3():
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=WEIGHT_SEED), strict=True)
    return net.to(DEV).eval()


def _frames16(n, h, w, depth, seed=0, over=True):
    """n frames of random samples below 2^depth; `over`: the first Y, U and V sample of frame 0 lie above it (they read as 2^depth - 1)."""
    npx = yuv.i420_bytes(h, w)
    s = np.random.RandomState(seed).randint(0, 1 << depth, size=(n, npx)).astype("<u2")
    if h == w == 64:                                      # every 12-bit code in Y, every 10-bit code in either chroma plane
        rng = np.random.RandomState(seed + 1)
        s[0, :4096] = rng.permutation(4096)
        s[0, 4096:5120] = rng.permutation(1024) << (depth - 10)
        s[0, 5120:] = rng.permutation(1024) << (depth - 10)
    elif over:
        ch, cw = yuv.chroma_hw(h, w)
        s[0, 0], s[0, h * w], s[0, h * w + ch * cw] = 1 << depth, 0xffff, (1 << depth) + 5
    return s.view(np.uint8)


def _gather(frames, h, w, idx, colour, depth, boff=0, expect=0):
    """The entry with the frames boff bytes off an allocation's start; the output buffer is poisoned: everything is written, nothing beyond."""
    lib = _lib()
    n, fb = frames.shape
    raw = torch.zeros(n * fb + 16, dtype=torch.uint8, device=DEV)
    raw[boff:boff + n * fb] = torch.from_numpy(frames.reshape(-1)).to(DEV)
    total = len(idx) * 3 * h * w
    out = torch.full((total + 64,), float("nan"), device=DEV)
    assert raw.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    rc = lib.savsr_video_gather_yuv420_16(raw.data_ptr() + boff, n, h, w, _idx(idx), len(idx), colour, depth, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    if expect:
        assert rc == expect and bool(torch.isnan(out).all())          # refused: nothing was launched
        return lib.savsr_last_error()
    assert rc == 0, lib.savsr_last_error()
    assert bool(torch.isnan(out[total:]).all())
    return out[:total].cpu().numpy().reshape(len(idx), 3, h, w)


def _quantize(x, colour, depth, boff=0, expect=0):
    lib = _lib()
    n, _, H, W = x.shape
    fb = yuv.i420_bytes(H, W, depth)
    src = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    out = torch.full((n * fb + 64 + boff,), 7, dtype=torch.uint8, device=DEV)
    assert src.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    rc = lib.savsr_video_quantize_yuv420_16(src.data_ptr(), n, H, W, colour, depth, out.data_ptr() + boff, _stream())
    torch.cuda.synchronize()
    if expect:
        assert rc == expect and bool((out == 7).all())
        return lib.savsr_last_error()
    assert rc == 0, lib.savsr_last_error()
    assert bool((out[:boff] == 7).all()) and bool((out[boff + n * fb:] == 7).all())
    return out[boff:boff + n * fb].cpu().numpy().reshape(n, fb)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# --------------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("h,w,boff", CASES)
def test_gather_16_bitwise(h, w, boff):
    for depth in DEPTHS:
        frames = _frames16(3, h, w, depth, seed=h + w + depth)
        for colour in COLOURS:
            ref = yuv.i420_to_rgb(frames, h, w, yuv.COLOURS[colour], depth)
            idx = [2, 0, 0, 1, 2, 2, 0]                   # repeated and out of order
            got = _gather(frames, h, w, idx, colour, depth, boff)
            assert np.array_equal(_bits(got), _bits(ref[idx])), (depth, colour)


def test_gather_16_index_lists_of_every_length():
    rng = np.random.RandomState(3)
    for (h, w), lengths in (((3, 5), range(1, MAX_SLOTS + 1)), ((8, 12), (1, 2, 7, 63, MAX_SLOTS))):
        frames = _frames16(5, h, w, 10, seed=h)
        ref = yuv.i420_to_rgb(frames, h, w, "bt709", 10)
        for n_idx in lengths:
            idx = [int(v) for v in rng.randint(0, 5, size=n_idx)]
            assert np.array_equal(_bits(_gather(frames, h, w, idx, 1, 10)), _bits(ref[idx])), n_idx


@pytest.mark.parametrize("H,W,boff", CASES)
def test_quantize_16_bitwise(H, W, boff):
    rng = np.random.RandomState(H * 3 + W)
    x = rng.uniform(-0.25, 1.25, size=(2, 3, H, W)).astype(np.float32)                 # below 0 and above 1 included
    x[0, :, 0, 0] = (-3.0, 0.5, 9.0)
    x[1, :, H - 1, W - 1] = (np.nan, 0.25, np.inf)
    x[1, 1, 0, 0] = np.nan
    for depth in DEPTHS:
        for colour in COLOURS:
            ref = yuv.rgb_to_i420(x, yuv.COLOURS[colour], depth)
            assert np.array_equal(_quantize(x, colour, depth, boff), ref), (depth, colour)


@pytest.mark.parametrize("depth", DEPTHS)
def test_quantize_16_exact_ties_round_half_to_even(depth):
    ties = grey_ties("bt601", depth)
    ns = sorted(ties)[:256]
    assert len(ns) >= 100 and any(n % 2 for n in ns) and any(n % 2 == 0 for n in ns)
    row = np.array([ties[n] for n in ns], np.float32)
    for W in (len(ns) // 4 * 4, len(ns) // 2 * 2 - 1):    # the vector and the 2 x 2 variant
        img = np.broadcast_to(row[None, None, None, :W], (1, 3, 4, W)).copy()
        ref = yuv.rgb_to_i420(img, "bt601", depth)
        assert np.array_equal(yuv.split_planes(ref, 4, W, depth)[0][0, 0], np.array([n + n % 2 for n in ns[:W]], np.uint16))      # half to even
        assert np.array_equal(_quantize(img, 0, depth), ref)


def _sad(frames, h, w, depth, boff=0):
    lib = _lib()
    n, fb = frames.shape
    raw = torch.zeros(n * fb + 16, dtype=torch.uint8, device=DEV)
    raw[boff:boff + n * fb] = torch.from_numpy(frames.reshape(-1)).to(DEV)
    sad = torch.full((n - 1 + 2,), -1, dtype=torch.int64, device=DEV)
    rc = lib.savsr_video_pair_sad_i420_16(raw.data_ptr() + boff, n, h, w, depth, sad.data_ptr(), _stream())
    assert rc == 0, lib.savsr_last_error()
    torch.cuda.synchronize()
    assert sad[n - 1:].tolist() == [-1, -1]
    return sad[:n - 1].cpu().numpy()


@pytest.mark.parametrize("h,w,boff", CASES + [(5, 4, 0)])          # (5 x 4: frames of 64 bytes, so 16-byte loads, whose 20 Y samples leave a tail of 4)
def test_pair_sad_16_equals_the_spec(h, w, boff):
    for depth in DEPTHS:
        frames = _frames16(4, h, w, depth, seed=h * w + depth)                          # (frame 0 holds samples above 2^depth - 1)
        ref = scenes.pair_sad(frames, "i420", (h, w), depth)
        assert ref.min() > 0
        assert np.array_equal(_sad(frames, h, w, depth, boff), ref), depth


def test_misaligned_and_bad_arguments_are_refused_without_a_launch():
    lib = _lib()
    h, w = 8, 12
    frames = _frames16(2, h, w, 10)
    x = np.zeros((1, 3, h, w), np.float32)
    assert b"video_gather_yuv420_16: frames must be 2-byte aligned" in _gather(frames, h, w, [0], 0, 10, boff=1, expect=-1)
    assert b"video_quantize_yuv420_16: out must be 2-byte aligned" in _quantize(x, 0, 10, boff=3, expect=-1)
    assert b"video_gather_yuv420_16: depth 8 (10 or 12" in _gather(frames, h, w, [0], 0, 8, expect=-1)
    assert b"video_gather_yuv420_16: colour 2 (0 .. 1: 10 and 12 bits are defined for limited range only)" in _gather(frames, h, w, [0], 2, 10, expect=-1)
    assert b"video_quantize_yuv420_16: colour 3" in _quantize(x, 3, 12, expect=-1)
    assert b"video_quantize_yuv420_16: depth 14" in _quantize(x, 0, 14, expect=-1)
    assert b"video_gather_yuv420_16: slot 1 names frame 2 of 2" in _gather(frames, h, w, [0, 2], 0, 10, expect=-1)
    assert b"video_gather_yuv420_16: 65 slots (1 .. 64)" in _gather(frames, h, w, [0] * 65, 0, 10, expect=-1)
    fd = torch.zeros(2 * yuv.i420_bytes(h, w, 10) + 16, dtype=torch.uint8, device=DEV)
    sad = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    assert lib.savsr_video_pair_sad_i420_16(fd.data_ptr() + 1, 2, h, w, 10, sad.data_ptr(), _stream()) == -1
    assert b"video_pair_sad_i420_16: frames must be 2-byte aligned" in lib.savsr_last_error()
    assert lib.savsr_video_pair_sad_i420_16(fd.data_ptr(), 2, h, w, 8, sad.data_ptr(), _stream()) == -1
    assert b"video_pair_sad_i420_16: depth 10 or 12" in lib.savsr_last_error()
    torch.cuda.synchronize()
    assert sad.tolist() == [-1] * 4
    # the public path names the pointer
    fb = yuv.i420_bytes(h, w, 10)
    odd = torch.zeros(9 * fb + 1, dtype=torch.uint8, device=DEV)[1:].view(9, fb)
    with pytest.raises(ValueError, match="10-bit I420 frames hold 16-bit samples: the base pointer 0x[0-9a-f]+ is not 2-byte aligned"):
        savsr_amd.pair_sad(odd, "i420", (h, w), depth=10)


def test_kernels_16_are_capturable():
    """No allocation, no host synchronisation: the three entries record into a hipGraph and replay."""
    lib = _lib()
    h, w, depth = 9, 14, 10
    frames = _frames16(3, h, w, depth, seed=1)
    fd = torch.from_numpy(frames).to(DEV)
    rgb = torch.zeros(2, 3, h, w, device=DEV)
    back = torch.zeros(2, yuv.i420_bytes(h, w, 12), dtype=torch.uint8, device=DEV)
    sad = torch.zeros(2, dtype=torch.int64, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            st = torch.cuda.current_stream().cuda_stream
            assert lib.savsr_video_gather_yuv420_16(fd.data_ptr(), 3, h, w, _idx([2, 0]), 2, 1, depth, rgb.data_ptr(), st) == 0
            assert lib.savsr_video_quantize_yuv420_16(rgb.data_ptr(), 2, h, w, 0, 12, back.data_ptr(), st) == 0
            assert lib.savsr_video_pair_sad_i420_16(fd.data_ptr(), 3, h, w, depth, sad.data_ptr(), st) == 0
        g.replay()
    s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    ref = yuv.i420_to_rgb(frames[[2, 0]], h, w, "bt709", depth)
    assert np.array_equal(_bits(rgb.cpu().numpy()), _bits(ref))
    assert np.array_equal(back.cpu().numpy(), yuv.rgb_to_i420(ref, "bt601", 12))
    assert np.array_equal(sad.cpu().numpy(), scenes.pair_sad(frames, "i420", (h, w), depth))


# ------------------------------------------------------------------------------------------------------------ the public interface
N, LR = 9, (8, 10)


def _video(depth, seed=0):
    """9 frames of 8 x 10 with in-range samples of the given depth ([N, bytes] uint8, host)."""
    h, w = LR
    if depth == 8:
        return np.random.RandomState(seed).randint(0, 256, size=(N, yuv.i420_bytes(h, w)), dtype=np.uint8)
    return _frames16(N, h, w, depth, seed=seed, over=False)


def _by_hand(net, frames, sc, depth, out_depth, colour="bt601", out_colour=None):
    """yuv.i420_to_rgb -> upscale_video on the float frames -> yuv.rgb_to_i420, the two conversions in numpy."""
    h, w = LR
    rgb = torch.from_numpy(yuv.i420_to_rgb(frames, h, w, colour, depth)).to(DEV)
    sr = net.upscale_video(rgb, scale=sc, out="float")
    return sr, yuv.rgb_to_i420(sr.cpu().numpy(), out_colour or colour, out_depth)


@pytest.mark.parametrize("sc", [(2.0, 2.0), (2.5, 3.0)])
def test_upscale_video_depths_equal_the_composition_by_hand(net3, sc):
    h, w = LR
    H, W = get_hw(h, w, sc)
    kw = dict(scale=sc, pixel_format="i420", size=(h, w), out="i420")
    f10, f8 = _video(10, seed=1), _video(8, seed=2)
    # 10 in, 10 out (out_depth = None: the input's), host and device frames
    sr, want = _by_hand(net3, f10, sc, 10, 10)
    got = net3.upscale_video(torch.from_numpy(f10), depth=10, out_depth=10, **kw)
    assert got.dtype == torch.uint8 and got.is_cuda and got.shape == (N, yuv.i420_bytes(H, W, 10)) == (N, 2 * yuv.i420_bytes(H, W))
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(net3.upscale_video(torch.from_numpy(f10).to(DEV), depth=10, **kw), got)
    assert torch.equal(net3.upscale_video(torch.from_numpy(f10), scale=sc, pixel_format="i420", size=(h, w), depth=10), sr)       # float out
    # 8 in, 10 out: the same network result as the 8-bit call, two more bits kept
    sr8, want = _by_hand(net3, f8, sc, 8, 10)
    got = net3.upscale_video(torch.from_numpy(f8), out_depth=10, **kw)
    assert np.array_equal(got.cpu().numpy(), want)
    q8 = net3.upscale_video(torch.from_numpy(f8), **kw)
    assert np.array_equal(q8.cpu().numpy(), yuv.rgb_to_i420(sr8.cpu().numpy()))          # (the defaults: today's bytes)
    y10, y8 = yuv.split_planes(want, H, W, 10)[0].astype(np.int64), yuv.split_planes(q8.cpu().numpy(), H, W)[0].astype(np.int64)
    assert np.abs(y10 - 4 * y8).max() <= 2 and (y10 != 4 * y8).any()
    # 10 in, 8 out; 12 in with BT.709, 10 out with BT.601
    assert np.array_equal(net3.upscale_video(torch.from_numpy(f10), depth=10, out_depth=8, **kw).cpu().numpy(), _by_hand(net3, f10, sc, 10, 8)[1])
    f12 = _video(12, seed=3)
    got = net3.upscale_video(torch.from_numpy(f12), depth=12, out_depth=10, colour="bt709", out_colour="bt601", **kw)
    assert np.array_equal(got.cpu().numpy(), _by_hand(net3, f12, sc, 12, 10, "bt709", "bt601")[1])
    # RGB in, 12 out
    u8 = torch.from_numpy(np.random.RandomState(4).randint(0, 256, size=(N, h, w, 3), dtype=np.uint8))
    f = net3.upscale_video(u8, scale=sc)
    got = net3.upscale_video(u8, scale=sc, out="i420", out_depth=12, out_colour="bt709")
    assert got.shape == (N, yuv.i420_bytes(H, W, 12)) and np.array_equal(got.cpu().numpy(), yuv.rgb_to_i420(f.cpu().numpy(), "bt709", 12))


def test_self_ensemble_and_fp16_with_depths_are_the_composition(net3):
    sc = (2.5, 3.0)
    kw = dict(scale=sc, pixel_format="i420", size=LR, out="i420")
    f10 = _video(10, seed=5)
    plain = net3.upscale_video(torch.from_numpy(f10), depth=10, **kw)
    net3.set_self_ensemble(True)
    try:
        got = net3.upscale_video(torch.from_numpy(f10), depth=10, out_depth=12, **kw)
        want = _by_hand(net3, f10, sc, 10, 12)[1]
        ens10 = net3.upscale_video(torch.from_numpy(f10), depth=10, **kw)
    finally:
        net3.set_self_ensemble(False)
    assert np.array_equal(got.cpu().numpy(), want) and not torch.equal(ens10, plain)     # (the switch acted)
    net3.set_precision("fp16")
    try:
        got = net3.upscale_video(torch.from_numpy(f10), depth=10, **kw)
        want = _by_hand(net3, f10, sc, 10, 10)[1]
    finally:
        net3.set_precision("fp32")
    assert np.array_equal(got.cpu().numpy(), want) and not torch.equal(got, plain)


def test_video_upscaler_with_depths_any_chunking_is_bitwise(net3):
    from savsr_amd import VideoUpscaler
    sc = (2.5, 3.0)
    H, W = get_hw(*LR, sc)
    for depth, out_depth in ((10, None), (8, 10), (12, 8)):
        frames = torch.from_numpy(_video(depth, seed=6 + depth))
        whole = net3.upscale_video(frames, scale=sc, out="i420", pixel_format="i420", size=LR, depth=depth, out_depth=out_depth)
        for chunk in (1, 4):
            up = VideoUpscaler(net3, sc, out="i420", pixel_format="i420", size=LR, depth=depth, out_depth=out_depth)
            parts = [up.push(frames[a:a + chunk] if chunk == 1 else frames[a:a + chunk].to(DEV)) for a in range(0, N, chunk)] + [up.finish()]
            assert all(p.dtype == torch.uint8 and p.shape[1] == yuv.i420_bytes(H, W, out_depth or depth) for p in parts)
            assert torch.equal(torch.cat(parts, 0), whole), (depth, out_depth, chunk)


def test_auto_cuts_at_depth_10_are_the_8_bit_videos(net3):
    from savsr_amd import VideoUpscaler
    v = SC.edited_video()
    h, w = SC.SCENE_HW
    y8 = yuv.rgb_to_i420((v.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2))
    y10 = torch.from_numpy((y8.astype("<u2") << 2).view(np.uint8))
    kw = dict(pixel_format="i420", size=(h, w))
    found = savsr_amd.detect_cuts(torch.from_numpy(y8), **kw)
    assert found == SC.SCENE_CUTS
    assert torch.equal(savsr_amd.pair_sad(y10, depth=10, **kw).cpu(), torch.from_numpy(scenes.pair_sad(y8, "i420", (h, w))))
    assert savsr_amd.detect_cuts(y10, depth=10, **kw) == found == savsr_amd.detect_cuts(y10.to(DEV), depth=10, **kw)
    whole = net3.upscale_video(y10, scale=2, out="i420", depth=10, cuts="auto", **kw)
    assert torch.equal(whole, net3.upscale_video(y10, scale=2, out="i420", depth=10, cuts=found, **kw))          # the 8-bit video's windows
    assert not torch.equal(whole, net3.upscale_video(y10, scale=2, out="i420", depth=10, **kw))
    up = VideoUpscaler(net3, 2, out="i420", depth=10, cuts="auto", **kw)
    got = torch.cat([up.push(y10[a:a + 4]) for a in range(0, len(v), 4)] + [up.finish()], 0)
    assert torch.equal(got, whole) and up.cuts == found


# ---------------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_high_depth_in_and_out(net3, tmp_path, capsys):
    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    h, w = LR
    sc = (2.0, 3.0)
    H, W = get_hw(h, w, sc)
    ckpt = tmp_path / "net.pth"
    sio.save_network(net3, str(ckpt))
    base = ["--scale", "2", "3", "--checkpoint", str(ckpt), "--chunk", "4"]

    def expected(frames, depth, out_depth):
        sr = net3.upscale_video(torch.from_numpy(frames), scale=sc, out="i420", pixel_format="i420", size=(h, w), depth=depth,
                                out_depth=out_depth).cpu().numpy()
        f = io.BytesIO()
        y4m.Y4MWriter(f, W, H, (30, 1), "p", y4m.scaled_aspect((1, 1), (h, w), (H, W)), depth=out_depth).write(sr)
        return f.getvalue()

    for depth, flag, out_depth in ((10, [], 10), (8, ["--out-depth", "10"], 10), (10, ["--out-depth", "8"], 8)):
        frames = _video(depth, seed=20 + depth)
        src, dst = tmp_path / f"lr{depth}.y4m", tmp_path / f"sr{depth}_{out_depth}.y4m"
        with open(src, "wb") as f:
            y4m.Y4MWriter(f, w, h, (30, 1), "p", (1, 1), depth=depth).write(frames)
        assert main(["-i", str(src), "-o", str(dst)] + flag + base) == 0
        assert f"upscaled {N} frames" in capsys.readouterr().out
        data = dst.read_bytes()
        tag = b"C420jpeg" if out_depth == 8 else f"C420p{out_depth}".encode()
        assert data.startswith(b"YUV4MPEG2 W30 H16 F30:1 Ip A2:3 " + tag + b"\n")
        assert data == expected(frames, depth, out_depth), (depth, out_depth)
