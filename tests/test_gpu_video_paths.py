"""Crossings of the video boundary that the per-format GPU files meet only by halves, all bit for bit: VideoUpscaler x the luma-only path
x cuts (given and "auto"), sitings through the streaming luma path, grey-scale frames x the self-ensemble, a colour network streamed
with auto cuts, and the empty result of a push that completes no window on a packed, a YUV and a luma-only upscaler.  N = 9 frames of
12 x 16 at x (2.5, 3) on the synthetic num_in_ch = 1 and 3 networks of tests/test_gpu_luma.py and tests/test_gpu_yuv_chroma.py."""
import numpy as np
import pytest
import torch

from savsr_amd import VideoUpscaler, detect_cuts, yuv
from savsr_amd.packing import get_hw
from tests.test_gpu_luma import DEV, LH, LW, SC, N, net1  # noqa: F401  (net1: the luma-only network fixture)
from tests.test_gpu_yuv_chroma import net3  # noqa: F401  (net3: the colour network fixture)

pytestmark = pytest.mark.gpu
LUMA_KW = dict(pixel_format="i422", size=(LH, LW), depth=12, siting="left", chroma_filter="bicubic")      # 12-bit 4:2:2 in ...
LUMA_OUT = dict(out="i420", out_depth=8, out_siting="left")                                                  # ... 8-bit 4:2:0 out


def _two_scenes(depth, layout, seed=0):
    """N frames of the layout whose frames 5 .. are bright and whose frames 0 .. 4 are dark (samples 16 .. 47 and 192 .. 223 on the 8-bit
    scale): pair (4, 5) differs by ~176 per sample, every other pair by ~11, so scdet's rule at its default threshold (25.5 per sample)
    finds the one cut."""
    rng = np.random.RandomState(seed)
    s = rng.randint(16, 48, size=(N, yuv.frame_bytes(LH, LW, 8, layout)))
    s[5:] += 176
    s <<= depth - 8
    return s.astype(np.uint8) if depth == 8 else s.astype("<u2").view(np.uint8)


def _streamed(up, frames, chunk):
    return torch.cat([up.push(torch.from_numpy(frames[a:a + chunk])) for a in range(0, N, chunk)] + [up.finish()], 0)


def test_luma_streamed_with_a_given_cut(net1):  # noqa: F811
    frames = _two_scenes(12, "422", seed=1)
    whole = net1.upscale_video(torch.from_numpy(frames), SC, cuts=[4], **LUMA_KW, **LUMA_OUT)
    got = _streamed(VideoUpscaler(net1, SC, cuts=[4], **LUMA_KW, **LUMA_OUT), frames, 4)
    assert torch.equal(got, whole)
    sr = net1.upscale_video(torch.from_numpy(frames), SC, out="float", cuts=[4], **LUMA_KW).cpu().numpy()
    assert np.array_equal(whole.cpu().numpy(), yuv.luma_only_frames(frames, LH, LW, sr, 12, 8, "422", "420", "left", "left"))
    assert not torch.equal(whole, net1.upscale_video(torch.from_numpy(frames), SC, **LUMA_KW, **LUMA_OUT))          # (the cut acted)


def test_luma_streamed_with_auto_cuts(net1):  # noqa: F811
    frames = _two_scenes(12, "422", seed=1)
    whole = net1.upscale_video(torch.from_numpy(frames), SC, cuts="auto", **LUMA_KW, **LUMA_OUT)
    up = VideoUpscaler(net1, SC, cuts="auto", **LUMA_KW, **LUMA_OUT)
    got = _streamed(up, frames, 2)
    cuts = detect_cuts(torch.from_numpy(frames), pixel_format="i422", size=(LH, LW), depth=12)
    assert cuts == [5] and up.cuts == cuts
    assert torch.equal(got, whole)
    assert torch.equal(whole, net1.upscale_video(torch.from_numpy(frames), SC, cuts=cuts, **LUMA_KW, **LUMA_OUT))


def test_grey_scale_with_the_self_ensemble(net1):  # noqa: F811
    frames = np.ascontiguousarray(_two_scenes(10, "420", seed=2)[:, :LH * LW * 2])
    kw = dict(pixel_format="y400", size=(LH, LW), depth=10, out="y400")
    plain = net1.upscale_video(torch.from_numpy(frames), SC, **kw)
    net1.set_self_ensemble(True)
    try:
        whole = net1.upscale_video(torch.from_numpy(frames), SC, **kw)
        up = VideoUpscaler(net1, SC, **kw)          # (reads the switch here)
    finally:
        net1.set_self_ensemble(False)
    assert torch.equal(_streamed(up, frames, 1), whole)
    H, W = get_hw(LH, LW, SC)
    assert whole.shape == (N, 2 * H * W) and whole.dtype == torch.uint8 and not torch.equal(whole, plain)


def test_colour_network_streamed_with_auto_cuts(net3):  # noqa: F811
    frames = _two_scenes(8, "420", seed=3)
    kw = dict(pixel_format="i420", size=(LH, LW), out="i444", out_depth=10, cuts="auto")
    whole = net3.upscale_video(torch.from_numpy(frames), SC, **kw)
    up = VideoUpscaler(net3, SC, **kw)
    assert torch.equal(_streamed(up, frames, 3), whole)
    assert up.cuts == [5] == detect_cuts(torch.from_numpy(frames), pixel_format="i420", size=(LH, LW))


@pytest.mark.parametrize("cuts", [None, "auto"])
def test_a_push_that_completes_no_window_returns_the_empty_result(net1, net3, cuts):  # noqa: F811
    H, W = get_hw(LH, LW, SC)
    rgb = torch.zeros(1, LH, LW, 3, dtype=torch.uint8)
    i420 = torch.from_numpy(_two_scenes(8, "420")[:1])
    i422 = torch.from_numpy(_two_scenes(12, "422")[:1])
    for up, chunk, shape, dtype in (
            (VideoUpscaler(net3, SC, cuts=cuts), rgb, (0, 3, H, W), torch.float32),
            (VideoUpscaler(net3, SC, out="uint8", cuts=cuts), rgb, (0, H, W, 3), torch.uint8),
            (VideoUpscaler(net3, SC, pixel_format="i420", size=(LH, LW), out="i444", out_depth=10, cuts=cuts), i420,
             (0, yuv.frame_bytes(H, W, 10, "444")), torch.uint8),
            (VideoUpscaler(net1, SC, cuts=cuts, **LUMA_KW, **LUMA_OUT), i422, (0, yuv.frame_bytes(H, W, 8, "420")), torch.uint8),
            (VideoUpscaler(net1, SC, out="float", cuts=cuts, **LUMA_KW), i422, (0, 1, H, W), torch.float32)):
        res = up.push(chunk)
        assert tuple(res.shape) == shape and res.dtype == dtype and res.device == DEV
        assert (up.seen, up.done) == (1, 0)
