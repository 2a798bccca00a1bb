"""The colour spaces of the raw-video path on the GPU: savsr_video_gather_yuv420 / savsr_video_quantize_yuv420 bit for bit against
savsr_amd/yuv.py for all four ids, the entries without a colour argument as their id 0, the refusals, and colour / out_colour through
SAVSR.upscale_video, the self-ensemble, VideoUpscaler and the CLI against the same calls composed by hand."""
import ctypes as C
import io
import re

import numpy as np
import pytest
import torch

from savsr_amd import y4m, yuv
from savsr_amd.packing import get_hw
from savsr_amd.utils import synth
from tests.video_cases import WEIGHT_SEED

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# 8 x 12 and 7 x 12 (an odd last row) take the vector variant from an aligned base, and the scalar one from a base one byte / one float off
SIZES = [(2, 2), (3, 5), (8, 12), (7, 12), (9, 11)]
CASES = [(h, w, 0) for h, w in SIZES] + [(8, 12, 1)]
IDS = range(len(yuv.COLOURS))


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


def _i420(n, h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=(n, yuv.i420_bytes(h, w)), dtype=np.uint8)


def _gather(frames, h, w, idx, colour, off=0):
    """colour = None: savsr_video_gather_i420.  Frames `off` bytes and output `off` floats from an allocation's start; the output is
    poisoned: everything is written, nothing beyond."""
    lib = _lib()
    n, fb = frames.shape
    raw = torch.zeros(n * fb + 16, dtype=torch.uint8, device=DEV)
    raw[off:off + n * fb] = torch.from_numpy(frames.reshape(-1)).to(DEV)
    total = len(idx) * 3 * h * w
    out = torch.full((total + 64 + off,), float("nan"), device=DEV)
    assert raw.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    if colour is None:
        rc = lib.savsr_video_gather_i420(raw.data_ptr() + off, n, h, w, _idx(idx), len(idx), out.data_ptr() + 4 * off, _stream())
    else:
        rc = lib.savsr_video_gather_yuv420(raw.data_ptr() + off, n, h, w, _idx(idx), len(idx), colour, out.data_ptr() + 4 * off, _stream())
    assert rc == 0, lib.savsr_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[:off]).all()) and bool(torch.isnan(out[off + total:]).all())
    return out[off:off + total].cpu().numpy().reshape(len(idx), 3, h, w)


def _quantize(x, colour, off=0):
    lib = _lib()
    n, _, H, W = x.shape
    fb = yuv.i420_bytes(H, W)
    src = torch.zeros(x.size + 8, device=DEV)
    src[off:off + x.size] = torch.from_numpy(x.reshape(-1)).to(DEV)
    out = torch.full((n * fb + 64 + off,), 7, dtype=torch.uint8, device=DEV)
    assert src.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    if colour is None:
        rc = lib.savsr_video_quantize_i420(src.data_ptr() + 4 * off, n, H, W, out.data_ptr() + off, _stream())
    else:
        rc = lib.savsr_video_quantize_yuv420(src.data_ptr() + 4 * off, n, H, W, colour, out.data_ptr() + off, _stream())
    assert rc == 0, lib.savsr_last_error()
    torch.cuda.synchronize()
    assert bool((out[:off] == 7).all()) and bool((out[off + n * fb:] == 7).all())
    return out[off:off + n * fb].cpu().numpy().reshape(n, fb)


def _rgb_in(n, H, W, seed):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-0.2, 1.2, size=(n, 3, H, W)).astype(np.float32)
    flat = x.reshape(-1)
    flat[rng.randint(0, flat.size, size=max(2, flat.size // 40))] = np.nan          # a few NaNs: they become 0
    x[0, :, :2, :2] = np.array((1.0, 0.0, 0.0), np.float32)[:, None, None]         # a red block: Cr = 255.5 at full range, the clip
    x[1, :, :2, :2] = np.array((0.0, 0.0, 1.0), np.float32)[:, None, None]         # a blue one: Cb = 255.5
    return x


@pytest.mark.parametrize("h,w,off", CASES)
def test_gather_yuv420_bitwise_and_the_old_entry_is_colour_0(h, w, off):
    n = 4
    frames = _i420(n, h, w, seed=h * 16 + w)                   # random bytes: limited-range legality is not assumed
    idx = [2, 2, 3, 2, 1, 0]                                   # a repeated and a reversed frame
    got = {c: _gather(frames, h, w, idx, c, off) for c in IDS}
    for c in IDS:
        ref = np.ascontiguousarray(yuv.i420_to_rgb(frames, h, w, colour=yuv.COLOURS[c])[idx])
        assert np.array_equal(got[c].view(np.uint32), ref.view(np.uint32)), yuv.COLOURS[c]
    assert np.array_equal(_gather(frames, h, w, idx, None, off).view(np.uint32), got[0].view(np.uint32))
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[0], got[2]) and not np.array_equal(got[1], got[3])


@pytest.mark.parametrize("H,W,off", CASES)
def test_quantize_yuv420_bitwise_and_the_old_entry_is_colour_0(H, W, off):
    x = _rgb_in(3, H, W, seed=H * 16 + W)
    got = {c: _quantize(x, c, off) for c in IDS}
    for c in IDS:
        assert np.array_equal(got[c], yuv.rgb_to_i420(x, colour=yuv.COLOURS[c])), yuv.COLOURS[c]
    assert np.array_equal(_quantize(x, None, off), got[0])
    for c in (2, 3):                                                                # full range: 255.5 -> 256 -> clipped, not wrapped
        _, u, v = yuv.split_planes(got[c], H, W)
        assert int(v[0, 0, 0]) == 255 and int(u[1, 0, 0]) == 255
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[0], got[2])


def test_colour_out_of_range_is_refused_before_the_device():
    lib = _lib()
    fd = torch.zeros(2 * yuv.i420_bytes(4, 4), dtype=torch.uint8, device=DEV)
    out = torch.zeros(2 * 48, device=DEV)
    x = torch.ones(48, device=DEV)
    q = torch.full((64,), 7, dtype=torch.uint8, device=DEV)
    st = _stream()
    for bad in (-1, 4):
        assert lib.savsr_video_gather_yuv420(fd.data_ptr(), 2, 4, 4, _idx([0, 1]), 2, bad, out.data_ptr(), st) == -1
        assert re.search(rb"video_gather_yuv420: colour %d \(0 \.\. 3\)" % bad, lib.savsr_last_error()), lib.savsr_last_error()
        assert lib.savsr_video_quantize_yuv420(x.data_ptr(), 1, 4, 4, bad, q.data_ptr(), st) == -1
        assert re.search(rb"video_quantize_yuv420: colour %d \(0 \.\. 3\)" % bad, lib.savsr_last_error()), lib.savsr_last_error()
    assert lib.savsr_video_gather_yuv420(None, 2, 4, 4, _idx([0]), 1, 1, out.data_ptr(), st) == -1
    assert b"video_gather_yuv420: null pointer" in lib.savsr_last_error()
    assert lib.savsr_video_gather_yuv420(fd.data_ptr(), 2, 4, 4, _idx([0, 2]), 2, 1, out.data_ptr(), st) == -1
    assert b"video_gather_yuv420: slot 1 names frame 2 of 2" in lib.savsr_last_error()
    assert lib.savsr_video_quantize_yuv420(x.data_ptr(), 0, 4, 4, 1, q.data_ptr(), st) == -1
    assert b"video_quantize_yuv420: n in 1 .. 65535, H, W >= 1" in lib.savsr_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0 and bool((q == 7).all())          # nothing was launched


# ------------------------------------------------------------------------------------------------------------ the public interface
N, H0, W0 = 9, 8, 10
PAIRS = [("bt709", None), ("bt601", "bt709"), ("bt601-full", "bt709")]


def _by_hand(net, frames, sc, a, b):
    rgb = torch.from_numpy(yuv.i420_to_rgb(frames, H0, W0, colour=a)).to(DEV)
    return yuv.rgb_to_i420(net.upscale_video(rgb, scale=sc, out="float").cpu().numpy(), colour=b or a)


@pytest.mark.parametrize("sc", [(2, 2), (2.5, 3)])
def test_upscale_video_colours_equal_the_composition(net3, sc):
    from savsr_amd import VideoUpscaler
    frames = _i420(N, H0, W0, seed=21)
    ft = torch.from_numpy(frames)
    kw = dict(scale=sc, pixel_format="i420", size=(H0, W0), out="i420")
    seen = []
    for a, b in PAIRS:
        want = _by_hand(net3, frames, sc, a, b)
        got = net3.upscale_video(ft, colour=a, out_colour=b, **kw)
        assert got.dtype == torch.uint8 and got.shape == (N, yuv.i420_bytes(*get_hw(H0, W0, sc)))
        assert np.array_equal(got.cpu().numpy(), want), (a, b)
        up = VideoUpscaler(net3, sc, out="i420", pixel_format="i420", size=(H0, W0), colour=a, out_colour=b)
        parts = [up.push(ft[i:i + 4]) for i in range(0, N, 4)] + [up.finish()]
        assert np.array_equal(torch.cat(parts, 0).cpu().numpy(), want), (a, b)
        seen.append(want)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    # the defaults: what colour="bt601" gives, which is the composition with yuv.py's defaults
    plain = net3.upscale_video(ft, **kw).cpu().numpy()
    assert np.array_equal(plain, net3.upscale_video(ft, colour="bt601", **kw).cpu().numpy())
    assert np.array_equal(plain, net3.upscale_video(ft, colour="bt601", out_colour="bt601", **kw).cpu().numpy())
    assert np.array_equal(plain, _by_hand(net3, frames, sc, "bt601", None))
    # RGB in, I420 out: out_colour alone
    u8 = np.random.RandomState(3).randint(0, 256, size=(N, H0, W0, 3), dtype=np.uint8)
    f = net3.upscale_video(torch.from_numpy(u8), scale=sc).cpu().numpy()
    got = net3.upscale_video(torch.from_numpy(u8), scale=sc, out="i420", out_colour="bt709-full").cpu().numpy()
    assert np.array_equal(got, yuv.rgb_to_i420(f, colour="bt709-full"))


def test_self_ensemble_takes_the_same_two_colours(net3):
    sc = (2.5, 3)
    frames = _i420(N, H0, W0, seed=22)
    a, b = PAIRS[0]
    net3.set_self_ensemble(True)
    try:
        want = _by_hand(net3, frames, sc, a, b)
        got = net3.upscale_video(torch.from_numpy(frames), scale=sc, pixel_format="i420", size=(H0, W0), out="i420", colour=a, out_colour=b)
        conv = net3.upscale_video(torch.from_numpy(frames), scale=sc, pixel_format="i420", size=(H0, W0), out="i420", colour="bt601",
                                  out_colour="bt709")
        want_conv = _by_hand(net3, frames, sc, "bt601", "bt709")
    finally:
        net3.set_self_ensemble(False)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(conv.cpu().numpy(), want_conv)
    assert not np.array_equal(want, _by_hand(net3, frames, sc, a, b))          # (the switch acted)


# ---------------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_colour_flags_end_to_end(net3, tmp_path, capsys):
    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    sc = (2.0, 2.0)
    H, W = get_hw(H0, W0, sc)
    frames = _i420(N, H0, W0, seed=23)
    src, dst, dst0, ckpt = tmp_path / "lr.y4m", tmp_path / "sr.y4m", tmp_path / "sr0.y4m", tmp_path / "net.pth"
    f = io.BytesIO()
    y4m.Y4MWriter(f, W0, H0, (30, 1), "p", (1, 1), colour_range="full").write(frames)
    src.write_bytes(f.getvalue())
    sio.save_network(net3, str(ckpt))
    base = ["-i", str(src), "--scale", "2", "--checkpoint", str(ckpt), "--chunk", "4"]

    def expected(a, b, tag):
        sr = net3.upscale_video(torch.from_numpy(frames), scale=sc, out="i420", pixel_format="i420", size=(H0, W0), colour=a, out_colour=b)
        g = io.BytesIO()
        y4m.Y4MWriter(g, W, H, (30, 1), "p", (1, 1), colour_range=tag).write(sr.cpu().numpy())
        return g.getvalue()

    # auto: the range from the tag, BT.601 at this size -> bt601-full in; the output tagged because the flags were given
    assert main(base + ["-o", str(dst), "--colour", "auto", "--out-colour", "bt709"]) == 0
    assert "colour bt601-full -> bt709" in capsys.readouterr().out
    want = expected("bt601-full", "bt709", "limited")
    assert want.startswith(b"YUV4MPEG2 W20 H16 F30:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n")
    assert dst.read_bytes() == want
    assert np.array_equal(np.frombuffer(want, np.uint8)[-yuv.i420_bytes(H, W):], _by_hand(net3, frames, sc, "bt601-full", "bt709")[-1])
    # without the flags: the tag is not followed, the header carries none, the bytes are bt601's
    assert main(base + ["-o", str(dst0)]) == 0
    assert "colour" not in capsys.readouterr().out
    want0 = expected("bt601", None, None)
    assert want0.startswith(b"YUV4MPEG2 W20 H16 F30:1 Ip A1:1 C420jpeg\n")
    assert dst0.read_bytes() == want0 and want0 != want
