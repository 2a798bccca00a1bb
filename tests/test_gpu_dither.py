"""Ordered dither on the GPU: savsr_video_quantize_u8_d / _yuvs_d / _luma_d bit for bit against their numpy specification
(savsr_amd/dither.py, yuv.rgb_to_i420 / yuv.unit_to_luma with dither=) and, at dither 0, against the bytes of the entries without _d;
then dither= of SAVSR.upscale_video, VideoUpscaler, the self-ensemble, the luma-only path, crop, surfaces, cuts and the CLI against the
specification applied to the out="float" result."""
import io
import os

import numpy as np
import pytest
import torch

from savsr_amd import active, y4m, yuv
from savsr_amd import dither as D
from savsr_amd.packing import get_hw
from savsr_amd.surface import Surface
from tests import dither_cases as DC
from tests.test_gpu_yuv_chroma import DEV, _cid, _lib, _stream, net3  # noqa: F401  (net3: the small-network fixture)

pytestmark = pytest.mark.gpu
E_ARG = -1
POISON = 7


def _sid(siting):
    return yuv.check_siting(siting) if siting is None or isinstance(siting, str) else siting


def _put(x):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    assert t.data_ptr() % 16 == 0
    return t


def _run(call, nbytes, boff=0, expect=0):
    """A quantiser entry into a poisoned buffer `boff` bytes off its alignment: the nbytes it owns are returned, nothing beyond is written;
    refused (`expect`): nothing is written at all and the message is returned."""
    lib = _lib()
    out = torch.full((nbytes + 64 + boff,), POISON, dtype=torch.uint8, device=DEV)
    assert out.data_ptr() % 16 == 0
    rc = call(lib, out.data_ptr() + boff)
    torch.cuda.synchronize()
    if expect:
        assert rc == expect and bool((out == POISON).all())
        return lib.savsr_last_error()
    assert rc == 0, lib.savsr_last_error()
    assert bool((out[:boff] == POISON).all()) and bool((out[boff + nbytes:] == POISON).all())
    return out[boff:boff + nbytes].cpu().numpy()


def _u8(x, dither, boff=0, expect=0, old=False):
    n, c, H, W = x.shape
    src = _put(x)
    if old:
        return _run(lambda lib, p: lib.savsr_video_quantize_u8(src.data_ptr(), n, c, H, W, p, _stream()), x.size, boff).reshape(n, H, W, c)
    got = _run(lambda lib, p: lib.savsr_video_quantize_u8_d(src.data_ptr(), n, c, H, W, dither, p, _stream()), x.size, boff, expect)
    return got if expect else got.reshape(n, H, W, c)


def _yuvs(x, colour, depth, chroma, siting, dither, boff=0, expect=0, old=False):
    n, _, H, W = x.shape
    fb = yuv.frame_bytes(H, W, depth if depth in DC.DEPTHS else 8, chroma if isinstance(chroma, str) else "420")
    cid = _cid(chroma) if isinstance(chroma, str) else chroma
    src = _put(x)
    if old:
        return _run(lambda lib, p: lib.savsr_video_quantize_yuvs(src.data_ptr(), n, H, W, colour, depth, cid, _sid(siting), p, _stream()),
                    n * fb, boff).reshape(n, fb)
    got = _run(lambda lib, p: lib.savsr_video_quantize_yuvs_d(src.data_ptr(), n, H, W, colour, depth, cid, _sid(siting), dither, p, _stream()),
               n * fb, boff, expect)
    return got if expect else got.reshape(n, fb)


def _luma(x, depth, dither, ofb, expect=0, old=False):
    """x [n, H, W] -> the n * ofb bytes of the frames (poisoned first: the bytes behind every Y plane must stay)."""
    n, H, W = x.shape
    src = _put(x)
    if old:
        return _run(lambda lib, p: lib.savsr_video_quantize_luma(src.data_ptr(), n, H, W, depth, p, ofb, _stream()), n * ofb).reshape(n, ofb)
    got = _run(lambda lib, p: lib.savsr_video_quantize_luma_d(src.data_ptr(), n, H, W, depth, dither, p, ofb, _stream()), n * ofb, 0, expect)
    return got if expect else got.reshape(n, ofb)


# ------------------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("H,W,c,n,boff", DC.U8_CASES)
def test_quantize_u8_d_bitwise(H, W, c, n, boff):
    x = DC.float_in(n, c, H, W)
    got = _u8(x, 1, boff)
    assert np.array_equal(got, D.rgb_to_u8(x, dither="ordered"))
    old = _u8(x, 0, boff, old=True)
    assert np.array_equal(_u8(x, 0, boff), old) and np.array_equal(old, D.rgb_to_u8(x))
    if H * W > 1:
        assert not np.array_equal(got, old)


@pytest.mark.parametrize("chroma", yuv.CHROMAS)
@pytest.mark.parametrize("H,W,off", DC.YUV_CASES)
def test_quantize_yuvs_d_bitwise(H, W, off, chroma):
    x = DC.float_in(2, 3, H, W)
    for depth in DC.DEPTHS:
        b = off * (1 if depth == 8 else 2)
        for siting in DC.sitings(chroma):
            for colour in DC.colours(depth):
                ref = yuv.rgb_to_i420(x, yuv.COLOURS[colour], depth, chroma, siting=siting, dither="ordered")
                assert np.array_equal(_yuvs(x, colour, depth, chroma, siting, 1, b), ref), (depth, siting, colour)
                old = _yuvs(x, colour, depth, chroma, siting, 0, b, old=True)
                assert np.array_equal(_yuvs(x, colour, depth, chroma, siting, 0, b), old), (depth, siting, colour)


@pytest.mark.parametrize("H,W", DC.LUMA_CASES)
def test_quantize_luma_d_bitwise(H, W):
    x = DC.float_in(2, 1, H, W)[:, 0]
    for depth in DC.DEPTHS:
        s = 1 if depth == 8 else 2
        ofb = yuv.frame_bytes(H, W, depth, "420")          # into the Y plane of I420 frames: the chroma planes behind it stay
        want = yuv.unit_to_luma(x, depth, dither="ordered")
        got = _luma(x, depth, 1, ofb)
        assert np.array_equal(got[:, :H * W * s], np.ascontiguousarray(want.astype(np.uint8 if s == 1 else "<u2")).reshape(2, -1).view(np.uint8)), depth
        assert bool((got[:, H * W * s:] == POISON).all())
        old = _luma(x, depth, 0, ofb, old=True)
        assert np.array_equal(_luma(x, depth, 0, ofb), old)
        assert np.array_equal(old[:, :H * W * s], np.ascontiguousarray(yuv.unit_to_luma(x, depth).astype(np.uint8 if s == 1 else "<u2")).reshape(2, -1).view(np.uint8))
    # [n, H, W, 1] uint8: Y planes with nothing between them
    assert np.array_equal(_luma(x, 8, 1, H * W).reshape(2, H, W), yuv.unit_to_luma(x, 8, dither="ordered"))
    assert np.array_equal(_luma(x, 8, 0, H * W), _luma(x, 8, 0, H * W, old=True))


def test_bad_arguments_are_refused_without_a_launch():
    lib = _lib()
    x3, x1 = np.zeros((1, 3, 8, 12), np.float32), np.zeros((1, 8, 12), np.float32)
    for d in (-1, 2):
        assert f"video_quantize_u8_d: dither {d} (0 = none, 1 = ordered)".encode() in _u8(x3, d, expect=E_ARG)
        assert f"video_quantize_yuvs_d: dither {d} (0 = none, 1 = ordered)".encode() in _yuvs(x3, 0, 8, "420", None, d, expect=E_ARG)
        assert f"video_quantize_luma_d: dither {d} (0 = none, 1 = ordered)".encode() in _luma(x1, 8, d, 144, expect=E_ARG)
    # what the entries without _d refuse, under the new names, dithered or not
    for d in (0, 1):
        assert b"video_quantize_yuvs_d: depth 9 (8, 10 or 12)" in _yuvs(x3, 0, 9, "420", None, d, expect=E_ARG)
        assert b"video_quantize_yuvs_d: colour 2 (0 .. 1: 10 and 12 bits are defined for limited range only)" in _yuvs(x3, 2, 10, "420", None, d, expect=E_ARG)
        assert b"video_quantize_yuvs_d: chroma 3 (0 = 4:2:0, 1 = 4:2:2, 2 = 4:4:4)" in _yuvs(x3, 0, 8, 3, None, d, expect=E_ARG)
        assert b"video_quantize_yuvs_d: siting 4 (0 = not modelled" in _yuvs(x3, 0, 8, "420", 4, d, expect=E_ARG)
        assert b"video_quantize_yuvs_d: out must be 2-byte aligned" in _yuvs(x3, 0, 12, "420", "left", d, boff=3, expect=E_ARG)
        assert b"video_quantize_luma_d: depth is 8, 10 or 12" in _luma(x1, 9, d, 144, expect=E_ARG)
        assert b"video_quantize_luma_d: out_frame_bytes is smaller than the Y plane" in _luma(x1, 8, d, 95, expect=E_ARG)
        bad = np.zeros((1, 4, 8, 12), np.float32)
        assert b"video_quantize_u8_d: n in 1 .. 65535, c in 1 .. 3, H, W >= 1" in _u8(bad, d, expect=E_ARG)
        out = torch.full((64,), POISON, dtype=torch.uint8, device=DEV)
        src = _put(x3)
        assert lib.savsr_video_quantize_u8_d(None, 1, 3, 2, 2, d, out.data_ptr(), _stream()) == E_ARG
        assert b"video_quantize_u8_d: null pointer" in lib.savsr_last_error()
        assert lib.savsr_video_quantize_yuvs_d(src.data_ptr(), 1, 2, 2, 0, 8, 0, 0, d, None, _stream()) == E_ARG
        assert b"video_quantize_yuvs_d: null pointer" in lib.savsr_last_error()
        assert lib.savsr_video_quantize_luma_d(None, 1, 2, 2, 8, d, out.data_ptr(), 4, _stream()) == E_ARG
        assert b"video_quantize_luma_d: null pointer" in lib.savsr_last_error()
        torch.cuda.synchronize()
        assert bool((out == POISON).all())


# ------------------------------------------------------------------------------------------------------------ the public interface
N, LR, SC_ = 9, (12, 20), (2.5, 1.5)


def _video_u8(seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=(N,) + LR + (3,), dtype=np.uint8)


@pytest.fixture(scope="module")
def ref(net3):  # noqa: F811
    """The shared reference, computed once: the uint8 video and its out="float" result, single pass and self-ensemble."""
    u8 = torch.from_numpy(_video_u8(seed=3))
    sr = net3.upscale_video(u8, scale=SC_, out="float").cpu().numpy()
    net3.set_self_ensemble(True)
    try:
        sr_e = net3.upscale_video(u8, scale=SC_, out="float").cpu().numpy()
    finally:
        net3.set_self_ensemble(False)
    return u8, sr, sr_e


def test_upscale_video_is_the_specification_applied_to_the_float_result(net3, ref):  # noqa: F811
    u8, sr, _ = ref
    H, W = get_hw(*LR, SC_)
    got = net3.upscale_video(u8, scale=SC_, out="uint8", dither="ordered")
    assert got.dtype == torch.uint8 and got.is_cuda and got.shape == (N, H, W, 3)
    assert np.array_equal(got.cpu().numpy(), D.rgb_to_u8(sr, dither="ordered"))
    for kw, args in ((dict(out="i420"), ("bt601", 8, "420", None)),
                     (dict(out="i420", out_depth=10), ("bt601", 10, "420", None)),
                     (dict(out="i444", out_colour="bt709"), ("bt709", 8, "444", None)),
                     (dict(out="i420", out_siting="left"), ("bt601", 8, "420", "left"))):
        got = net3.upscale_video(u8, scale=SC_, dither="ordered", **kw).cpu().numpy()
        assert np.array_equal(got, yuv.rgb_to_i420(sr, *args, dither="ordered")), kw
        assert not np.array_equal(got, yuv.rgb_to_i420(sr, *args)), kw


def test_dither_none_is_the_call_without_the_argument(net3, ref):  # noqa: F811
    u8, sr, _ = ref
    for out, want in (("uint8", D.rgb_to_u8(sr)), ("i420", yuv.rgb_to_i420(sr))):
        a = net3.upscale_video(u8, scale=SC_, out=out, dither=None)
        assert torch.equal(a, net3.upscale_video(u8, scale=SC_, out=out)) and np.array_equal(a.cpu().numpy(), want)
    with pytest.raises(ValueError, match="out = 'float' has nothing to quantise"):
        net3.upscale_video(u8, scale=SC_, dither="ordered")
    with pytest.raises(ValueError, match="dither = 'bayer': None or one of ordered"):
        net3.upscale_video(u8, scale=SC_, out="uint8", dither="bayer")
    with pytest.raises(TypeError):
        net3.upscale_video(u8, SC_, "reflection", "uint8", "rgb", None, None, 10.0, "bt601", None, 8, None, None, None, None, None, 24, "keep", None, None,
                           5, "ordered")          # keyword only


def test_self_ensemble_merges_in_fp32_and_dithers_after(net3, ref):  # noqa: F811
    u8, sr, sr_e = ref
    net3.set_self_ensemble(True)
    try:
        got_u8 = net3.upscale_video(u8, scale=SC_, out="uint8", dither="ordered").cpu().numpy()
        got_yuv = net3.upscale_video(u8, scale=SC_, out="i420", dither="ordered").cpu().numpy()
        plain = net3.upscale_video(u8, scale=SC_, out="uint8").cpu().numpy()          # (the fused merge, undithered, as ever)
    finally:
        net3.set_self_ensemble(False)
    assert np.array_equal(got_u8, D.rgb_to_u8(sr_e, dither="ordered")) and not np.array_equal(got_u8, D.rgb_to_u8(sr, dither="ordered"))
    assert np.array_equal(got_yuv, yuv.rgb_to_i420(sr_e, dither="ordered"))
    assert np.array_equal(plain, D.rgb_to_u8(sr_e))


def test_luma_only_network_dithers_y_and_keeps_the_resampled_chroma():
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.utils import synth
    net1 = SAVSR(num_in_ch=1, num_feat=32)
    net1.load_state_dict(synth.synth_state_dict(synth.manifest_of(net1.state_dict()), seed=3), strict=True)
    net1 = net1.to(DEV).eval()
    h, w = LR
    H, W = get_hw(h, w, SC_)
    f = torch.from_numpy(np.random.RandomState(5).randint(0, 256, size=(N, yuv.frame_bytes(h, w)), dtype=np.uint8))
    kw = dict(scale=SC_, pixel_format="i420", size=LR, chroma_filter="bicubic")
    luma = net1.upscale_video(f, out="float", **kw).cpu().numpy()
    assert luma.shape == (N, 1, H, W)
    plain = net1.upscale_video(f, out="i420", **kw).cpu().numpy()
    got = net1.upscale_video(f, out="i420", dither="ordered", **kw).cpu().numpy()
    assert np.array_equal(got[:, :H * W].reshape(N, H, W), yuv.unit_to_luma(luma[:, 0], 8, dither="ordered"))
    assert np.array_equal(got[:, H * W:], plain[:, H * W:]) and not np.array_equal(got[:, :H * W], plain[:, :H * W])
    got = net1.upscale_video(f, out="uint8", dither="ordered", **kw).cpu().numpy()
    assert np.array_equal(got[..., 0], yuv.unit_to_luma(luma[:, 0], 8, dither="ordered"))


# ----------------------------------------------------------------------------------------------------------------------- composition
def test_video_upscaler_any_chunking_is_bitwise(net3, ref):  # noqa: F811
    from savsr_amd import VideoUpscaler
    u8, sr, _ = ref
    whole = net3.upscale_video(u8, scale=SC_, out="i420", dither="ordered")
    assert np.array_equal(whole.cpu().numpy(), yuv.rgb_to_i420(sr, dither="ordered"))
    for chunk in (1, 4, N):
        up = VideoUpscaler(net3, SC_, out="i420", dither="ordered")
        parts = [up.push(u8[a:a + chunk]) for a in range(0, N, chunk)] + [up.finish()]
        assert torch.equal(torch.cat(parts, 0), whole), chunk
    with pytest.raises(ValueError, match="out = 'float' has nothing to quantise"):
        VideoUpscaler(net3, SC_, dither="ordered")


def test_crop_is_the_hand_crop_with_the_same_dither(net3, ref):  # noqa: F811
    u8 = ref[0]
    rect = (2, 4, 8, 12)
    hand = torch.from_numpy(np.ascontiguousarray(active.crop_frames(u8.numpy(), rect)))
    want = net3.upscale_video(hand, scale=SC_, out="uint8", dither="ordered")
    drop = net3.upscale_video(u8, scale=SC_, out="uint8", dither="ordered", crop=rect, bars="drop")
    assert torch.equal(drop, want)
    keep = net3.upscale_video(u8, scale=SC_, out="uint8", dither="ordered", crop=rect, bars="keep")
    full = active.insert_frames(want.cpu().numpy(), active.place(rect, *LR, SC_, None), "uint8")
    assert np.array_equal(keep.cpu().numpy(), full)
    assert not torch.equal(drop, net3.upscale_video(hand, scale=SC_, out="uint8"))


def test_out_surface_packs_the_dithered_planar_result(net3, ref):  # noqa: F811
    import savsr_amd
    u8, sr, _ = ref
    H, W = get_hw(*LR, SC_)
    surf = Surface.nv12(pitch_align=64)
    planar = net3.upscale_video(u8, scale=SC_, out="i420", dither="ordered")
    got = net3.upscale_video(u8, scale=SC_, out="i420", dither="ordered", out_surface=surf)
    assert torch.equal(got, savsr_amd.pack_surface(planar, surf, "i420", (H, W)))


def test_cuts_are_the_scenes_alone_concatenated(net3, ref):  # noqa: F811
    u8 = ref[0]
    kw = dict(scale=SC_, out="i420", dither="ordered", padding="replicate")
    got = net3.upscale_video(u8, cuts=[4], **kw)
    assert torch.equal(got, torch.cat([net3.upscale_video(u8[:4], **kw), net3.upscale_video(u8[4:], **kw)], 0))
    assert not torch.equal(got, net3.upscale_video(u8, **kw))


# ------------------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_png_folder_and_y4m_write_the_bytes_of_the_api_call(net3, ref, tmp_path):  # noqa: F811
    from PIL import Image
    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    u8, sr, _ = ref
    H, W = get_hw(*LR, SC_)
    src, ckpt = tmp_path / "lr", tmp_path / "net.pth"
    src.mkdir()
    names = [f"im{i:03d}.png" for i in range(N)]
    for i, nm in enumerate(names):
        Image.fromarray(u8[i].numpy()).save(src / nm)
    sio.save_network(net3, str(ckpt))
    common = ["--scale", str(SC_[0]), str(SC_[1]), "--checkpoint", str(ckpt), "--chunk", "4"]
    for flag, want in ((["--dither", "ordered"], D.rgb_to_u8(sr, dither="ordered")), ([], D.rgb_to_u8(sr))):
        dst = tmp_path / ("sr_" + "_".join(flag).strip("-"))
        assert main(["-i", str(src), "-o", str(dst)] + flag + common) == 0
        assert sorted(os.listdir(dst)) == names
        for i, nm in enumerate(names):
            assert np.array_equal(np.asarray(Image.open(dst / nm)), want[i]), (flag, nm)
    # .y4m -> .y4m
    h, w = LR
    frames = np.random.RandomState(8).randint(0, 256, size=(N, yuv.frame_bytes(h, w)), dtype=np.uint8)
    f = io.BytesIO()
    y4m.Y4MWriter(f, w, h, (30, 1), "p", (1, 1)).write(frames)
    (tmp_path / "lr.y4m").write_bytes(f.getvalue())
    for flag, d in ((["--dither", "ordered"], "ordered"), ([], None)):
        out = tmp_path / f"sr_{d}.y4m"
        assert main(["-i", str(tmp_path / "lr.y4m"), "-o", str(out)] + flag + common) == 0
        api = net3.upscale_video(torch.from_numpy(frames), scale=SC_, out="i420", pixel_format="i420", size=LR, dither=d).cpu().numpy()
        with open(out, "rb") as fh:
            r = y4m.Y4MReader(fh)
            assert (r.width, r.height) == (W, H)
            assert np.array_equal(np.concatenate(list(r.chunks(16)), 0), api), flag
