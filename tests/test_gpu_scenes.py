"""GPU checks of the scene-cut path: the three savsr_video_pair_sad_* entries against the numpy specification (exact integers), the segment
property of upscale_video(cuts=...) (bit for bit the per-segment calls), cuts="auto", VideoUpscaler with cuts under any chunking, the CLI."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import savsr_amd
from savsr_amd import scenes, y4m, yuv
from savsr_amd.packing import get_hw
from savsr_amd.utils import synth
from savsr_amd.video import PADDING_MODES, check_length
from tests import scene_cases as SC
from tests.video_cases import WEIGHT_SEED

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = [(7, 9), (8, 12), (5, 3), (181, 319), (720, 1280)]
T = 7


def _lib():
    from savsr_amd import _lib as L
    return L.load()


@pytest.fixture(scope="module")
def net3():
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=WEIGHT_SEED), strict=True)
    return net.to(DEV).eval()


def _raw_sad(kind, dev_frames, n, c, h, w):
    """One entry of the C ABI on a device tensor's pointer; the score buffer is poisoned first (the entry zeroes it itself) and has a
    guard cell behind it (nothing beyond n - 1 entries is written)."""
    lib = _lib()
    out = torch.full((n,), -12345, dtype=torch.int64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    if kind == "u8":
        rc = lib.savsr_video_pair_sad_u8(dev_frames.data_ptr(), n, c, h, w, out.data_ptr(), st)
    elif kind == "i420":
        rc = lib.savsr_video_pair_sad_i420(dev_frames.data_ptr(), n, h, w, out.data_ptr(), st)
    else:
        rc = lib.savsr_video_pair_sad_f32(dev_frames.data_ptr(), n, c, h, w, out.data_ptr(), st)
    assert rc == 0, lib.savsr_last_error()
    got = out.cpu().numpy()
    assert got[n - 1] == -12345
    return got[:n - 1]


def _offset_copy(host: np.ndarray, off_bytes: int) -> torch.Tensor:
    """The array on the device, `off_bytes` past the start of an allocation (allocations are at least 256-byte aligned)."""
    flat = torch.from_numpy(np.ascontiguousarray(host)).reshape(-1)
    off = off_bytes // flat.element_size()
    buf = torch.empty(flat.numel() + off + 64, dtype=flat.dtype, device=DEV)
    assert buf.data_ptr() % 256 == 0
    view = buf[off:off + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() == buf.data_ptr() + off_bytes
    return view


# ---------------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("c", [1, 2, 3])
@pytest.mark.parametrize("h,w", SIZES)
def test_pair_sad_u8_equals_the_spec(h, w, c):
    v = np.random.RandomState(h * 7 + w + c).randint(0, 256, size=(9, h, w, c), dtype=np.uint8)
    v[4] = v[3]                                                                   # an identical pair: 0
    v[6] = 255 - v[5]
    want = scenes.pair_sad(v)
    dv = torch.from_numpy(v).to(DEV)
    off = _offset_copy(v, 1)                                                      # the base pointer one byte off: the unaligned path
    for n in range(1, 10):
        assert np.array_equal(_raw_sad("u8", dv, n, c, h, w), want[:n - 1]), (h, w, c, n)
        assert np.array_equal(_raw_sad("u8", off, n, c, h, w), want[:n - 1]), (h, w, c, n, "offset")
        got = savsr_amd.pair_sad(dv[:n])
        assert got.dtype == torch.int64 and got.device == dv.device and np.array_equal(got.cpu().numpy(), want[:n - 1])
    assert np.array_equal(savsr_amd.pair_sad(torch.from_numpy(v)).cpu().numpy(), want)          # host frames


@pytest.mark.parametrize("h,w", SIZES)
def test_pair_sad_i420_equals_the_spec(h, w):
    fb = yuv.i420_bytes(h, w)
    v = np.random.RandomState(h + w).randint(0, 256, size=(9, fb), dtype=np.uint8)
    v[2, :h * w] = v[1, :h * w]                                                   # same luma, other chroma: 0
    want = scenes.pair_sad(v, "i420", (h, w))
    assert want[1] == 0
    dv = torch.from_numpy(v).to(DEV)
    off = _offset_copy(v, 1)
    for n in range(1, 10):
        assert np.array_equal(_raw_sad("i420", dv, n, 0, h, w), want[:n - 1]), (h, w, n)
        assert np.array_equal(_raw_sad("i420", off, n, 0, h, w), want[:n - 1]), (h, w, n, "offset")
        assert np.array_equal(savsr_amd.pair_sad(dv[:n], "i420", (h, w)).cpu().numpy(), want[:n - 1])


def _float_video(n, c, h, w, seed):
    rng = np.random.RandomState(seed)
    v = rng.uniform(-0.25, 1.25, size=(n, c, h, w)).astype(np.float32)
    flat = v.reshape(-1)
    k = flat.size
    ties = (rng.randint(0, 255, size=k // 5).astype(np.float32) + np.float32(0.5)) / np.float32(255)      # x.5 / 255
    flat[rng.randint(0, k, size=ties.size)] = ties
    exact = rng.randint(0, 256, size=k // 5).astype(np.float32) / np.float32(255)                          # a byte's own value
    flat[rng.randint(0, k, size=exact.size)] = exact
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, -3.0, 7.0, 0.5, 1e-30, -1e-30], np.float32)
    where = rng.permutation(min(k, 100000))[:min(k, 4 * special.size)]
    flat[where] = np.resize(special, where.size)
    return v


@pytest.mark.parametrize("c", [1, 2, 3])
@pytest.mark.parametrize("h,w", SIZES)
def test_pair_sad_f32_equals_the_spec(h, w, c):
    v = _float_video(9, c, h, w, seed=h + 3 * w + c)
    assert np.isnan(v).any() and (v < 0).any() and (v > 1).any()
    want = scenes.pair_sad(v)
    dv = torch.from_numpy(v).to(DEV)
    off = _offset_copy(v, 4)                                                      # one float off a 16-byte boundary
    for n in range(1, 10):
        assert np.array_equal(_raw_sad("f32", dv, n, c, h, w), want[:n - 1]), (h, w, c, n)
        assert np.array_equal(_raw_sad("f32", off, n, c, h, w), want[:n - 1]), (h, w, c, n, "offset")
        assert np.array_equal(savsr_amd.pair_sad(dv[:n]).cpu().numpy(), want[:n - 1])


# every planar layout at two depths and packed uint8, at 5 x 3 (an odd frame stride: the one-sample form) and 16 x 32 (strides and bases
# are 16-byte multiples: the vector form); one float case
_KINDS = [(fmt, depth, h, w) for fmt in ("y400", "i420", "i422", "i444") for depth in (8, 10) for h, w in ((5, 3), (16, 32))]
_KINDS += [("rgb", 8, 5, 3), ("rgb", 8, 16, 32), ("float", 8, 5, 3)]


@pytest.mark.parametrize("fmt,depth,h,w", _KINDS)
def test_public_pair_sad_of_every_frame_kind_equals_the_spec(fmt, depth, h, w):
    """savsr_amd.pair_sad picks the C entry from the frame kind (planar colour: _yuvp; packed and grey-scale: _u8; float: _f32)."""
    rng = np.random.RandomState(h + 5 * w + depth + len(fmt))
    if fmt == "float":
        v, kw = _float_video(3, 3, h, w, seed=11), {}
    elif fmt == "rgb":
        v, kw = rng.randint(0, 256, size=(3, h, w, 3), dtype=np.uint8), {}
    else:
        kw = dict(pixel_format=fmt, size=(h, w), depth=depth)
        samples = yuv.frame_bytes(h, w, 8, savsr_amd.video.layout_of(fmt))
        if depth == 8:
            v = rng.randint(0, 256, size=(3, samples), dtype=np.uint8)
        else:          # 16-bit samples, some above the depth's range (they count as the largest one)
            v = rng.randint(0, 1 << depth, size=(3, samples)).astype("<u2")
            v[rng.rand(3, samples) < 0.05] = 0xFFFF
            v = v.view(np.uint8).reshape(3, -1)
    want = scenes.pair_sad(v, **kw)
    got = savsr_amd.pair_sad(torch.from_numpy(v).to(DEV), **kw)
    assert got.dtype == torch.int64 and got.shape == (2,) and np.array_equal(got.cpu().numpy(), want), (fmt, depth, h, w)


def test_pair_sad_covers_every_byte_value_against_every_other():
    a = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, 1)               # a[i, j] = i
    pair = np.stack([a, a.T], 0)                                                  # b[i, j] = j
    want = int(np.abs(np.arange(256)[:, None] - np.arange(256)[None, :]).sum())
    assert scenes.pair_sad(pair[..., None]).tolist() == [want]
    dv = torch.from_numpy(pair).to(DEV)
    assert _raw_sad("u8", dv, 2, 1, 256, 256).tolist() == [want]
    assert _raw_sad("u8", _offset_copy(pair, 1), 2, 1, 256, 256).tolist() == [want]
    fl = pair.astype(np.float32) / np.float32(255)                                # every byte's float value quantises back to it
    assert _raw_sad("f32", torch.from_numpy(fl).to(DEV), 2, 1, 256, 256).tolist() == [want]
    i420 = np.concatenate([pair.reshape(2, -1), np.zeros((2, 2 * 128 * 128), np.uint8)], 1)
    assert _raw_sad("i420", torch.from_numpy(i420).to(DEV), 2, 0, 256, 256).tolist() == [want]
    # the largest sum of a 720 x 1280 x 3 pair
    big = torch.zeros(2, 720, 1280, 3, dtype=torch.uint8, device=DEV)
    big[1] = 255
    assert savsr_amd.pair_sad(big).tolist() == [255 * 3 * 720 * 1280]


def test_pair_sad_refuses_bad_arguments():
    lib = _lib()
    v = torch.zeros(2, 4, 4, 3, dtype=torch.uint8, device=DEV)
    out = torch.zeros(2, dtype=torch.int64, device=DEV)
    for args in ((0, 2, 3, 4, 4, out.data_ptr()), (v.data_ptr(), 2, 3, 4, 4, 0), (v.data_ptr(), 0, 3, 4, 4, out.data_ptr()),
                 (v.data_ptr(), 2, 4, 4, 4, out.data_ptr()), (v.data_ptr(), 2, 3, 0, 4, out.data_ptr()),
                 (v.data_ptr(), 2, 3, 4, 4, out.data_ptr() + 4)):
        assert lib.savsr_video_pair_sad_u8(*args, None) != 0
        assert lib.savsr_last_error()
    assert lib.savsr_video_pair_sad_i420(v.data_ptr(), 2, 0, 4, out.data_ptr(), None) != 0
    assert lib.savsr_video_pair_sad_f32(0, 2, 3, 4, 4, out.data_ptr(), None) != 0
    torch.cuda.synchronize()
    assert out.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------------------- the segment property
def _video_u8(n, h, w, c=3, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=(n, h, w, c), dtype=np.uint8)


def _by_segments(net, frames, cuts, padding, **kw):
    """The definition: upscale_video on every segment alone, its padding "replicate" exactly when check_length refuses the segment."""
    n = int(frames.shape[0])
    parts = []
    edges = [0] + list(cuts) + [n]
    for a, b in zip(edges[:-1], edges[1:]):
        try:
            check_length(b - a, net.num_frame, padding)
            mode = padding
        except ValueError:
            mode = "replicate"
        parts.append(net.upscale_video(frames[a:b], padding=mode, **kw))
    return torch.cat(parts, 0)


LENGTHS = (1, 2, 3, 4, 6, 7, 9)                       # segments shorter than every mode needs, at each mode's limit, and long ones
CUTS = list(np.cumsum(LENGTHS)[:-1])                  # [1, 3, 6, 10, 16, 23] of 32 frames


@pytest.mark.parametrize("padding", PADDING_MODES)
def test_cuts_equal_the_per_segment_calls_bitwise(net3, padding):
    u8 = torch.from_numpy(_video_u8(sum(LENGTHS), 10, 12, seed=21))
    got = net3.upscale_video(u8, scale=3, padding=padding, cuts=CUTS)
    want = _by_segments(net3, u8, CUTS, padding, scale=3)
    assert got.shape == want.shape and torch.equal(got, want)
    assert not torch.equal(got, net3.upscale_video(u8, scale=3, padding=padding))               # the cuts change frames
    for out in ("uint8", "i420"):
        got = net3.upscale_video(u8.to(DEV), scale=(2.5, 2), padding=padding, out=out, cuts=tuple(CUTS))
        assert torch.equal(got, _by_segments(net3, u8, CUTS, padding, scale=(2.5, 2), out=out)), out
    fl = (u8.to(DEV).float() / 255).permute(0, 3, 1, 2).contiguous()                           # float frames
    assert torch.equal(net3.upscale_video(fl, scale=2, padding=padding, cuts=[4, 5, 20]),
                       _by_segments(net3, fl, [4, 5, 20], padding, scale=2))


@pytest.mark.parametrize("padding", PADDING_MODES)
def test_cuts_with_i420_frames_bitwise(net3, padding):
    h, w = 10, 12
    v = torch.from_numpy(np.random.RandomState(23).randint(0, 256, size=(sum(LENGTHS), yuv.i420_bytes(h, w)), dtype=np.uint8))
    for out in ("float", "i420"):
        got = net3.upscale_video(v, scale=2, padding=padding, out=out, pixel_format="i420", size=(h, w), cuts=CUTS)
        assert torch.equal(got, _by_segments(net3, v, CUTS, padding, scale=2, out=out, pixel_format="i420", size=(h, w))), out


def test_cuts_with_self_ensemble_bitwise(net3):
    u8 = torch.from_numpy(_video_u8(14, 8, 10, seed=25))
    cuts = [1, 3, 7]                                  # 1, 2, 4 and 7 frames
    net3.set_self_ensemble(True)
    try:
        for out in ("float", "uint8"):
            got = net3.upscale_video(u8, scale=2, padding="reflection", out=out, cuts=cuts)
            assert torch.equal(got, _by_segments(net3, u8, cuts, "reflection", scale=2, out=out)), out
    finally:
        net3.set_self_ensemble(False)


def test_cuts_in_fp16_mode_bitwise(net3):
    u8 = torch.from_numpy(_video_u8(sum(LENGTHS), 10, 12, seed=27))
    net3.set_precision("fp16")
    try:
        for padding in ("reflection", "circle"):
            got = net3.upscale_video(u8, scale=3, padding=padding, out="uint8", cuts=CUTS)
            assert torch.equal(got, _by_segments(net3, u8, CUTS, padding, scale=3, out="uint8")), padding
    finally:
        net3.set_precision("fp32")


def test_short_videos_pass_with_cuts_and_are_refused_without(net3):
    u8 = torch.from_numpy(_video_u8(3, 8, 8, seed=29))
    with pytest.raises(ValueError, match="too few"):
        net3.upscale_video(u8, scale=2, padding="circle")
    assert torch.equal(net3.upscale_video(u8, scale=2, padding="circle", cuts=[]), net3.upscale_video(u8, scale=2, padding="replicate"))
    assert torch.equal(net3.upscale_video(u8[:1], scale=2, cuts="auto"), net3.upscale_video(u8[:1], scale=2, padding="replicate"))
    with pytest.raises(ValueError):
        net3.upscale_video(u8, scale=2, cuts=[3])


# ----------------------------------------------------------------------------------------------------------------------------- auto
def test_auto_finds_the_cuts_of_an_edited_video(net3):
    """Three scenes (tests/scene_cases.py: independent smooth textures drifting a pixel per frame under +-2 levels of noise), 9 + 4 + 8
    frames of 24 x 32.  The specification's own scores, in per cent of the largest change, at the default threshold of 10: the smaller
    of the two cuts 31.61, the largest of the 18 other pairs 2.90; the first scene continued over all 21 frames: at most 2.21."""
    v = SC.edited_video()
    S = v[0].size
    sc = SC.scores(scenes.pair_sad(v), S)
    cut_min = min(sc[k - 1] for k in SC.SCENE_CUTS)
    rest_max = max(s for k, s in enumerate(sc, 1) if k not in SC.SCENE_CUTS)
    print(f"edited video: min cut score {cut_min:.2f}, max non-cut score {rest_max:.2f}")
    assert cut_min >= 2 * 10.0 and rest_max <= 10.0 / 2
    u8 = torch.from_numpy(v)
    assert savsr_amd.detect_cuts(u8) == SC.SCENE_CUTS == scenes.cuts_from_sad(scenes.pair_sad(v), S)
    assert savsr_amd.detect_cuts(u8.to(DEV), threshold=40) == []
    for padding in ("reflection", "circle"):
        got = net3.upscale_video(u8, scale=2, padding=padding, out="uint8", cuts="auto")
        assert torch.equal(got, net3.upscale_video(u8, scale=2, padding=padding, out="uint8", cuts=SC.SCENE_CUTS))
        assert torch.equal(got, _by_segments(net3, u8, SC.SCENE_CUTS, padding, scale=2, out="uint8"))
    fl = (u8.to(DEV).float() / 255).permute(0, 3, 1, 2).contiguous()
    assert savsr_amd.detect_cuts(fl) == SC.SCENE_CUTS
    assert torch.equal(net3.upscale_video(fl, scale=2, cuts="auto"), net3.upscale_video(fl, scale=2, cuts=SC.SCENE_CUTS))
    # one scene over the same 21 frames: nothing found, and the call is the call without cuts
    one = SC.scene(SC.SCENE_SEEDS[0], 21, *SC.SCENE_HW)
    sc1 = SC.scores(scenes.pair_sad(one), S)
    print(f"one scene: max score {max(sc1):.2f}")
    assert max(sc1) <= 10.0 / 2
    u1 = torch.from_numpy(one)
    assert savsr_amd.detect_cuts(u1) == []
    for out in ("float", "uint8"):
        assert torch.equal(net3.upscale_video(u1, scale=2, out=out, cuts="auto"), net3.upscale_video(u1, scale=2, out=out))
    # a lower threshold is a parameter like any other: the decisions are the specification's
    low = scenes.cuts_from_sad(scenes.pair_sad(v), S, 2.5)
    assert len(low) > 2 and savsr_amd.detect_cuts(u8, threshold=2.5) == low
    assert torch.equal(net3.upscale_video(u8, scale=2, cuts="auto", scene_threshold=2.5), net3.upscale_video(u8, scale=2, cuts=low))


# ------------------------------------------------------------------------------------------------------------------------ streaming
@pytest.mark.parametrize("padding", PADDING_MODES)
def test_video_upscaler_with_cuts_any_chunking_is_bitwise(net3, padding):
    from savsr_amd import VideoUpscaler
    v = SC.edited_video()
    u8 = torch.from_numpy(v)
    n = len(v)
    found = savsr_amd.detect_cuts(u8)
    assert found == SC.SCENE_CUTS
    whole = net3.upscale_video(u8, scale=2, padding=padding, out="uint8", cuts="auto")
    for chunk in (1, 2, 5, 16, n):
        for cuts in ("auto", SC.SCENE_CUTS):
            up = VideoUpscaler(net3, 2, padding, out="uint8", cuts=cuts)
            parts = []
            for a in range(0, n, chunk):
                parts.append(up.push(u8[a:a + chunk]))
                assert up.cuts == [k for k in found if k < min(n, a + chunk)]
            parts.append(up.finish())
            assert torch.equal(torch.cat(parts, 0), whole), (padding, chunk, cuts)
            assert up.cuts == found
    explicit = [2, 3, 10, 20]                          # other cuts than the detector's, float frames on the GPU, float out
    fl = (u8.to(DEV).float() / 255).permute(0, 3, 1, 2).contiguous()
    want = net3.upscale_video(fl, scale=2, padding=padding, cuts=explicit)
    for chunk in (1, 4, n):
        up = VideoUpscaler(net3, 2, padding, cuts=explicit)
        got = torch.cat([up.push(fl[a:a + chunk]) for a in range(0, n, chunk)] + [up.finish()], 0)
        assert torch.equal(got, want), (padding, chunk)
    up = VideoUpscaler(net3, 2, padding, cuts=[5, n])  # a cut at the final length: refused when the video ends
    up.push(u8)
    with pytest.raises(ValueError):
        up.finish()


def test_video_upscaler_with_cuts_i420_and_float_auto(net3):
    from savsr_amd import VideoUpscaler
    v = SC.edited_video()
    h, w = SC.SCENE_HW
    yv = torch.from_numpy(yuv.rgb_to_i420((v.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2)))
    found = savsr_amd.detect_cuts(yv, pixel_format="i420", size=(h, w))
    assert found == SC.SCENE_CUTS == scenes.cuts_from_sad(scenes.pair_sad(yv.numpy(), "i420", (h, w)), h * w)
    whole = net3.upscale_video(yv, scale=2, out="i420", pixel_format="i420", size=(h, w), cuts="auto")
    assert torch.equal(whole, net3.upscale_video(yv, scale=2, out="i420", pixel_format="i420", size=(h, w), cuts=found))
    for chunk in (1, 5, 16):
        up = VideoUpscaler(net3, 2, out="i420", pixel_format="i420", size=(h, w), cuts="auto")
        got = torch.cat([up.push(yv[a:a + chunk]) for a in range(0, len(v), chunk)] + [up.finish()], 0)
        assert torch.equal(got, whole) and up.cuts == found
    fl = (torch.from_numpy(v).to(DEV).float() / 255).permute(0, 3, 1, 2).contiguous()
    whole = net3.upscale_video(fl, scale=2, cuts="auto")
    for chunk in (2, 7):
        up = VideoUpscaler(net3, 2, cuts="auto")
        got = torch.cat([up.push(fl[a:a + chunk]) for a in range(0, len(v), chunk)] + [up.finish()], 0)
        assert torch.equal(got, whole) and up.cuts == SC.SCENE_CUTS


def test_video_upscaler_with_cuts_memory_stays_flat(net3):
    from savsr_amd import VideoUpscaler
    lengths = [20, 3, 37, 2, 18, 40, 6, 24, 30, 20]                              # 200 frames, 9 cuts
    v = SC.edited_video(seeds=range(40, 50), lengths=lengths, hw=(64, 64))
    cuts = list(np.cumsum(lengths)[:-1])
    u8 = torch.from_numpy(v)
    assert savsr_amd.detect_cuts(u8) == cuts
    up = VideoUpscaler(net3, 2, "reflection", out="uint8", cuts="auto")
    seen, n_out = [], 0
    for a in range(0, 200, 5):
        n_out += up.push(u8[a:a + 5]).shape[0]
        torch.cuda.synchronize()
        assert up._buf.shape[0] <= 5 + T - 1                                      # the chunk and at most num_frame - 1 past frames
        if a >= 100:                                       # after warm-up: every (unit size, stream) graph has been captured
            seen.append(torch.cuda.memory_allocated(DEV))
    n_out += up.finish().shape[0]
    assert n_out == 200 and up.cuts == cuts
    assert max(seen) - min(seen) <= 1 << 20, (min(seen), max(seen))


# ------------------------------------------------------------------------------------------------------------------------------ CLI
def test_cli_folder_with_auto_cuts(net3, tmp_path, capsys):
    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    v = SC.edited_video()
    src, dst, lst = tmp_path / "lr", tmp_path / "sr", tmp_path / "cuts.txt"
    src.mkdir()
    names = [f"im{i:03d}.png" for i in range(len(v))]
    for i, nm in enumerate(names):
        Image.fromarray(v[i]).save(src / nm)
    ckpt = tmp_path / "net.pth"
    sio.save_network(net3, str(ckpt))
    assert main(["-i", str(src), "-o", str(dst), "--scale", "2", "--checkpoint", str(ckpt), "--chunk", "4", "--cuts", "auto",
                 "--cuts-out", str(lst)]) == 0
    line = capsys.readouterr().out
    assert f"upscaled {len(v)} frames" in line and line.rstrip().endswith(", 3 scenes")
    assert lst.read_text() == "9\n13\n"
    ref = net3.upscale_video(torch.from_numpy(v), scale=2, out="uint8", cuts="auto").cpu().numpy()
    for i, nm in enumerate(names):
        assert np.array_equal(np.asarray(Image.open(dst / nm)), ref[i]), nm
    # the list just written, given back with @FILE and a padding the short scene cannot serve: the same frames as the explicit call
    dst2 = tmp_path / "sr2"
    assert main(["-i", str(src), "-o", str(dst2), "--scale", "2", "--checkpoint", str(ckpt), "--padding", "circle", "--cuts", f"@{lst}"]) == 0
    ref = net3.upscale_video(torch.from_numpy(v), scale=2, padding="circle", out="uint8", cuts=SC.SCENE_CUTS).cpu().numpy()
    for i, nm in enumerate(names):
        assert np.array_equal(np.asarray(Image.open(dst2 / nm)), ref[i]), nm
    with pytest.raises(ValueError):                                              # a cut beyond the folder: refused before the GPU runs
        main(["-i", str(src), "-o", str(tmp_path / "sr3"), "--scale", "2", "--checkpoint", str(ckpt), "--cuts", "9,21"])


def test_cli_y4m_with_auto_cuts(net3, tmp_path, capsys):
    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    v = SC.edited_video()
    h, w = SC.SCENE_HW
    frames = yuv.rgb_to_i420((v.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2))
    f = io.BytesIO()
    y4m.Y4MWriter(f, w, h, (30, 1), "p", (1, 1)).write(frames)
    src, dst, lst, ckpt = tmp_path / "lr.y4m", tmp_path / "sr.y4m", tmp_path / "cuts.txt", tmp_path / "net.pth"
    src.write_bytes(f.getvalue())
    sio.save_network(net3, str(ckpt))
    assert main(["-i", str(src), "-o", str(dst), "--scale", "2", "--checkpoint", str(ckpt), "--chunk", "5", "--cuts", "auto",
                 "--cuts-out", str(lst)]) == 0
    assert capsys.readouterr().out.rstrip().endswith(", 3 scenes")
    assert lst.read_text() == "9\n13\n"
    H, W = get_hw(h, w, (2, 2))
    sr = net3.upscale_video(torch.from_numpy(frames), scale=2, out="i420", pixel_format="i420", size=(h, w), cuts="auto").cpu().numpy()
    g = io.BytesIO()
    y4m.Y4MWriter(g, W, H, (30, 1), "p", y4m.scaled_aspect((1, 1), (h, w), (H, W))).write(sr)
    assert dst.read_bytes() == g.getvalue()
