"""Raw YUV 4:2:0 on the GPU: savsr_video_gather_i420 / savsr_video_quantize_i420 bit for bit against their numpy restatement
(savsr_amd/yuv.py, which tests/test_yuv.py pins to the REFERENCE), SAVSR.upscale_video / VideoUpscaler / the self-ensemble with I420
frames in and out against the same calls on converted frames, and the Y4M paths of the CLI end to end."""
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from savsr_amd import y4m, yuv
from savsr_amd.packing import get_hw
from savsr_amd.utils import synth
from tests.video_cases import PADDINGS, WEIGHT_SEED

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
GOLDEN_SIZES = [(2, 2), (3, 5), (8, 10), (9, 14), (17, 33)]
# (5 x 3, 8 x 12, 64 x 64, 18 x 20: with the golden ones the shapes of the other layouts' and depths' tests -- an odd last row and column, the
# vector path, more than one workgroup of it, and with the 2-byte offset a w % 4 == 0 image on the scalar path)
SIZES = GOLDEN_SIZES + [(5, 3), (8, 12), (64, 64), (18, 20), (180, 320), (181, 319), (720, 1280), (715, 1273)]
OFFSETS = [(0, 0), (1, 0), (4, 0), (0, 1), (0, 4), (1, 1), (2, 0)]  # (bytes on the uint8 side, floats on the fp32 side)


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


def _gather(frames: np.ndarray, h, w, idx, boff=0, foff=0):
    """savsr_video_gather_i420 with the frames boff bytes and the output foff floats off an allocation's start; the output buffer is
    poisoned: everything is written, nothing beyond."""
    lib = _lib()
    n, fb = frames.shape
    raw = torch.zeros(n * fb + 16, dtype=torch.uint8, device=DEV)
    raw[boff:boff + n * fb] = torch.from_numpy(frames.reshape(-1)).to(DEV)
    total = len(idx) * 3 * h * w
    out = torch.full((total + 64 + foff,), float("nan"), device=DEV)
    assert raw.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    rc = lib.savsr_video_gather_i420(raw.data_ptr() + boff, n, h, w, _idx(idx), len(idx), out.data_ptr() + 4 * foff, _stream())
    assert rc == 0, lib.savsr_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[:foff]).all()) and bool(torch.isnan(out[foff + total:]).all())
    return out[foff:foff + total].cpu().numpy().reshape(len(idx), 3, h, w)


@pytest.mark.parametrize("h,w", SIZES)
def test_gather_i420_bitwise(h, w):
    n = 3 if h * w > 100000 else 5
    frames = _i420(n, h, w, seed=h + w)
    ref = yuv.i420_to_rgb(frames, h, w)
    rng = np.random.RandomState(h)
    for boff, foff in OFFSETS if h * w < 100000 else OFFSETS[:4]:
        idx = [int(v) for v in rng.randint(0, n, size=6)] + [0, 0, n - 1]           # repeats
        got = _gather(frames, h, w, idx, boff, foff)
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(ref[idx]).view(np.uint32)), (boff, foff)


def test_gather_i420_every_byte_value_and_the_reference_golden():
    gold = np.load(os.path.join(ROOT, "tests", "golden", "yuv_outputs.npz"))
    frames = gold["in/table/i420"]                       # all 256 Y values against a 16-step (U, V) grid
    for boff, foff in ((0, 0), (1, 1)):
        got = _gather(frames, 256, 256, [0], boff, foff)
        assert np.array_equal(got.view(np.uint32), yuv.i420_to_rgb(frames, 256, 256).view(np.uint32))
        assert float(np.abs(got.astype(np.float64) - gold["in/table/rgb"]).max()) <= 2e-6
    h, w = 16, 48                                        # every byte value in every plane (768 Y, 192 U, 192 V samples)
    fr = (np.arange(yuv.i420_bytes(h, w)) * 7 % 256).astype(np.uint8)[None]
    for p in yuv.split_planes(fr, h, w):
        assert len(np.unique(p)) >= 192
    assert len(np.unique(yuv.split_planes(fr, h, w)[0])) == 256
    assert np.array_equal(_gather(fr, h, w, [0]).view(np.uint32), yuv.i420_to_rgb(fr, h, w).view(np.uint32))


def test_gather_i420_refuses_bad_arguments():
    lib = _lib()
    fd = torch.zeros(2 * yuv.i420_bytes(4, 4), dtype=torch.uint8, device=DEV)
    out = torch.zeros(64 * 48, device=DEV)
    st = _stream()
    assert lib.savsr_video_gather_i420(fd.data_ptr(), 2, 4, 4, _idx([0, 2]), 2, out.data_ptr(), st) == -1
    assert b"video_gather_i420: slot 1 names frame 2 of 2" in lib.savsr_last_error()
    assert lib.savsr_video_gather_i420(fd.data_ptr(), 2, 4, 4, _idx([-1]), 1, out.data_ptr(), st) == -1
    assert b"slot 0 names frame -1 of 2" in lib.savsr_last_error()
    assert lib.savsr_video_gather_i420(fd.data_ptr(), 2, 4, 4, _idx([0] * 65), 65, out.data_ptr(), st) == -1
    assert b"video_gather_i420: 65 slots (1 .. 64)" in lib.savsr_last_error()
    assert lib.savsr_video_gather_i420(fd.data_ptr(), 2, 4, 4, None, 1, out.data_ptr(), st) == -1
    assert b"null index list" in lib.savsr_last_error()
    assert lib.savsr_video_gather_i420(fd.data_ptr(), 2, 0, 4, _idx([0]), 1, out.data_ptr(), st) == -1
    assert b"video_gather_i420: h, w, n_frames >= 1" in lib.savsr_last_error()
    assert lib.savsr_video_gather_i420(None, 2, 4, 4, _idx([0]), 1, out.data_ptr(), st) == -1
    assert b"video_gather_i420: null pointer" in lib.savsr_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                  # nothing was launched


def _quantize(x: np.ndarray, boff=0, foff=0):
    lib = _lib()
    n, _, H, W = x.shape
    fb = yuv.i420_bytes(H, W)
    src = torch.zeros(x.size + 8, device=DEV)
    src[foff:foff + x.size] = torch.from_numpy(x.reshape(-1)).to(DEV)
    out = torch.full((n * fb + 64 + boff,), 7, dtype=torch.uint8, device=DEV)
    assert src.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    rc = lib.savsr_video_quantize_i420(src.data_ptr() + 4 * foff, n, H, W, out.data_ptr() + boff, _stream())
    assert rc == 0, lib.savsr_last_error()
    torch.cuda.synchronize()
    assert bool((out[:boff] == 7).all()) and bool((out[boff + n * fb:] == 7).all())
    return out[boff:boff + n * fb].cpu().numpy().reshape(n, fb)


@pytest.mark.parametrize("H,W", SIZES)
def test_quantize_i420_bitwise(H, W):
    n = 2
    rng = np.random.RandomState(H * 3 + W)
    x = rng.uniform(-0.25, 1.25, size=(n, 3, H, W)).astype(np.float32)             # below 0 and above 1 included
    x[0, :, 0, 0] = (-3.0, 0.5, 9.0)
    ref = yuv.rgb_to_i420(x)
    for boff, foff in OFFSETS if H * W < 100000 else OFFSETS[:4]:
        assert np.array_equal(_quantize(x, boff, foff), ref), (boff, foff)


def _grey_ties():
    """Grey levels v (float32) on which the float32 Y of the restatement is exactly k + 0.5: searched among the neighbours of
    (k + 0.5 - 16) / 219."""
    found = {}
    for k in range(16, 235):
        v0 = np.float32((k + 0.5 - 16.0) / 219.0)
        cand = [v0]
        for _ in range(48):
            cand.append(np.nextafter(cand[-1], np.float32(2.0)))
        lo = v0
        for _ in range(48):
            lo = np.nextafter(lo, np.float32(-1.0))
            cand.append(lo)
        cand = np.array(cand, np.float32)
        img = np.broadcast_to(cand[None, None, None, :], (1, 3, 2, cand.size)).copy()
        y = yuv.ycbcr_f32(img)[0][0, 0]
        hit = np.nonzero(y == np.float32(k + 0.5))[0]
        if hit.size:
            found[k] = cand[hit[0]]
    return found


def test_quantize_i420_exact_ties_round_half_to_even():
    ties = _grey_ties()
    assert len(ties) >= 100, len(ties)                   # (most k have a float32 grey level that lands on the tie exactly)
    ks = sorted(ties)
    row = np.array([ties[k] for k in ks], np.float32)
    for W in (len(ks) // 4 * 4, len(ks) // 2 * 2 - 1):   # the vector and the scalar variant
        img = np.broadcast_to(row[None, None, None, :W], (1, 3, 4, W)).copy()
        y_f = yuv.ycbcr_f32(img)[0]
        assert np.array_equal(y_f[0, 0], np.array(ks[:W], np.float32) + np.float32(0.5))          # known ties
        ref = yuv.rgb_to_i420(img)
        want = np.array([k if k % 2 == 0 else k + 1 for k in ks[:W]], np.uint8)                   # half to even
        assert np.array_equal(yuv.split_planes(ref, 4, W)[0][0, 0], want)
        assert np.array_equal(_quantize(img), ref)


def test_quantize_i420_refuses_bad_arguments():
    lib = _lib()
    x = torch.zeros(3 * 16, device=DEV)
    out = torch.zeros(64, dtype=torch.uint8, device=DEV)
    st = _stream()
    assert lib.savsr_video_quantize_i420(x.data_ptr(), 0, 4, 4, out.data_ptr(), st) == -1
    assert b"video_quantize_i420: n in 1 .. 65535, H, W >= 1" in lib.savsr_last_error()
    assert lib.savsr_video_quantize_i420(x.data_ptr(), 65536, 4, 4, out.data_ptr(), st) == -1
    assert lib.savsr_video_quantize_i420(x.data_ptr(), 1, 4, 0, out.data_ptr(), st) == -1
    assert lib.savsr_video_quantize_i420(x.data_ptr(), 1, 4, 4, None, st) == -1
    assert b"video_quantize_i420: null pointer" in lib.savsr_last_error()


def test_kernels_are_capturable():
    """No allocation, no host synchronisation: both entries record into a hipGraph and replay."""
    lib = _lib()
    h, w = 9, 14
    frames = _i420(3, h, w, seed=1)
    fd = torch.from_numpy(frames).to(DEV)
    rgb = torch.zeros(2, 3, h, w, device=DEV)
    back = torch.zeros(2, yuv.i420_bytes(h, w), dtype=torch.uint8, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            st = torch.cuda.current_stream().cuda_stream
            assert lib.savsr_video_gather_i420(fd.data_ptr(), 3, h, w, _idx([2, 0]), 2, rgb.data_ptr(), st) == 0
            assert lib.savsr_video_quantize_i420(rgb.data_ptr(), 2, h, w, back.data_ptr(), st) == 0
        g.replay()
    s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    ref = yuv.i420_to_rgb(frames[[2, 0]], h, w)
    assert np.array_equal(rgb.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(back.cpu().numpy(), yuv.rgb_to_i420(ref))


# ------------------------------------------------------------------------------------------------------------ the public interface
def _rgb_of(frames: np.ndarray, h, w) -> torch.Tensor:
    return torch.from_numpy(yuv.i420_to_rgb(frames, h, w)).to(DEV)


@pytest.mark.parametrize("h,w,sc", [(16, 20, (2.3125, 2.25)), (15, 21, (2.2, 3.0))])
def test_upscale_video_i420_equals_the_rgb_path_on_converted_frames(net3, h, w, sc):
    H, W = get_hw(h, w, sc)
    assert H % 2 == 1 and W % 2 == 1                         # an odd HR size at an asymmetric scale
    n = 9
    frames = _i420(n, h, w, seed=h)
    ref = net3.upscale_video(_rgb_of(frames, h, w), scale=sc, out="float")
    got = net3.upscale_video(torch.from_numpy(frames), scale=sc, out="float", pixel_format="i420", size=(h, w))           # host frames
    assert got.shape == (n, 3, H, W) and torch.equal(got, ref)
    got = net3.upscale_video(torch.from_numpy(frames).to(DEV), scale=sc, out="float", pixel_format="i420", size=(h, w))
    assert torch.equal(got, ref)
    q = net3.upscale_video(torch.from_numpy(frames), scale=sc, out="i420", pixel_format="i420", size=(h, w))
    assert q.dtype == torch.uint8 and q.shape == (n, yuv.i420_bytes(H, W)) and q.is_cuda
    want = yuv.rgb_to_i420(ref.cpu().numpy())
    assert np.array_equal(q.cpu().numpy(), want)
    # RGB in / I420 out, and I420 in / uint8 RGB out
    u8 = np.random.RandomState(1).randint(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    f = net3.upscale_video(torch.from_numpy(u8), scale=sc)
    assert np.array_equal(net3.upscale_video(torch.from_numpy(u8), scale=sc, out="i420").cpu().numpy(), yuv.rgb_to_i420(f.cpu().numpy()))
    assert torch.equal(net3.upscale_video(torch.from_numpy(frames), scale=sc, out="uint8", pixel_format="i420", size=(h, w)),
                       net3.upscale_video(_rgb_of(frames, h, w), scale=sc, out="uint8"))


@pytest.mark.parametrize("padding", PADDINGS)
def test_video_upscaler_i420_any_chunking_is_bitwise(net3, padding):
    from savsr_amd import VideoUpscaler
    n, h, w, sc = 13, 9, 11, (3, 2)
    frames = torch.from_numpy(_i420(n, h, w, seed=5))
    whole = net3.upscale_video(frames, scale=sc, padding=padding, out="i420", pixel_format="i420", size=(h, w))
    for chunk in (1, 3, 7, n):
        up = VideoUpscaler(net3, sc, padding, out="i420", pixel_format="i420", size=(h, w))
        parts = [up.push(frames[a:a + chunk] if chunk != 3 else frames[a:a + chunk].to(DEV)) for a in range(0, n, chunk)]
        parts.append(up.finish())
        assert all(p.dtype == torch.uint8 and p.dim() == 2 for p in parts)
        assert torch.equal(torch.cat(parts, 0), whole), (padding, chunk)
    up = VideoUpscaler(net3, sc, padding, pixel_format="i420", size=(h, w))
    got = torch.cat([up.push(frames[a:a + 4]) for a in range(0, n, 4)] + [up.finish()], 0)
    assert torch.equal(got, net3.upscale_video(frames, scale=sc, padding=padding, pixel_format="i420", size=(h, w)))


def test_self_ensemble_i420_is_the_composition(net3):
    """I420 in: converted once to fp32 planar RGB, then the fp32 ensemble path; I420 out: the fp32 merge, then the quantisation."""
    n, h, w, sc = 8, 9, 12, (2.0, 3.5)
    frames = _i420(n, h, w, seed=8)
    net3.set_self_ensemble(True)
    try:
        ref = net3.upscale_video(_rgb_of(frames, h, w), scale=sc, out="float")
        f = net3.upscale_video(torch.from_numpy(frames), scale=sc, out="float", pixel_format="i420", size=(h, w))
        q = net3.upscale_video(torch.from_numpy(frames), scale=sc, out="i420", pixel_format="i420", size=(h, w))
        u8 = np.random.RandomState(2).randint(0, 256, size=(n, h, w, 3), dtype=np.uint8)
        fu = net3.upscale_video(torch.from_numpy(u8), scale=sc)
        qu = net3.upscale_video(torch.from_numpy(u8), scale=sc, out="i420")
    finally:
        net3.set_self_ensemble(False)
    plain = net3.upscale_video(_rgb_of(frames, h, w), scale=sc, out="float")
    assert not torch.equal(ref, plain)                       # (the switch acted)
    assert torch.equal(f, ref)
    assert np.array_equal(q.cpu().numpy(), yuv.rgb_to_i420(ref.cpu().numpy()))
    assert np.array_equal(qu.cpu().numpy(), yuv.rgb_to_i420(fu.cpu().numpy()))


# ---------------------------------------------------------------------------------------------------------------------------- CLI
def _y4m_bytes(frames, h, w, fps=(30, 1), aspect=(1, 1)):
    f = io.BytesIO()
    y4m.Y4MWriter(f, w, h, fps, "p", aspect).write(frames)
    return f.getvalue()


def _expected_y4m(net, frames, h, w, sc, fps, aspect):
    H, W = get_hw(h, w, sc)
    sr = net.upscale_video(torch.from_numpy(frames), scale=sc, out="i420", pixel_format="i420", size=(h, w)).cpu().numpy()
    f = io.BytesIO()
    y4m.Y4MWriter(f, W, H, fps, "p", y4m.scaled_aspect(aspect, (h, w), (H, W))).write(sr)
    return f.getvalue()


def test_cli_y4m_file_to_y4m_file(net3, tmp_path, capsys):
    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    n, h, w, sc = 10, 12, 14, (3.5, 2.0)
    frames = _i420(n, h, w, seed=11)
    src, dst, ckpt = tmp_path / "lr.y4m", tmp_path / "sr.y4m", tmp_path / "net.pth"
    src.write_bytes(_y4m_bytes(frames, h, w))
    sio.save_network(net3, str(ckpt))
    assert main(["-i", str(src), "-o", str(dst), "--scale", "3.5", "2", "--checkpoint", str(ckpt), "--chunk", "3"]) == 0
    assert f"upscaled {n} frames" in capsys.readouterr().out
    want = _expected_y4m(net3, frames, h, w, sc, (30, 1), (1, 1))
    assert want.startswith(b"YUV4MPEG2 W28 H42 F30:1 Ip A7:4 C420jpeg\n")
    assert dst.read_bytes() == want


def test_cli_y4m_through_stdin_and_stdout_of_a_child_process(net3, tmp_path):
    from savsr_amd import io as sio
    n, h, w, sc = 9, 11, 13, (2.0, 2.0)
    frames = _i420(n, h, w, seed=12)
    ckpt = tmp_path / "net.pth"
    sio.save_network(net3, str(ckpt))
    r = subprocess.run([sys.executable, "-m", "savsr_amd.upscale", "-i", "-", "-o", "-", "--scale", "2", "--checkpoint", str(ckpt), "--chunk", "4"],
                       input=_y4m_bytes(frames, h, w, (25, 1), (0, 0)), capture_output=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert r.stdout == _expected_y4m(net3, frames, h, w, sc, (25, 1), (0, 0))
    assert f"upscaled {n} frames" in r.stderr.decode()
    # a pipe's length is unknown: a video too short for the window is refused when the input ends
    r = subprocess.run([sys.executable, "-m", "savsr_amd.upscale", "-i", "-", "-o", "-", "--scale", "2", "--checkpoint", str(ckpt)],
                       input=_y4m_bytes(frames[:3], h, w), capture_output=True, cwd=ROOT, timeout=600)
    assert r.returncode != 0 and "video has 3 frames: too few for a 7-frame 'reflection' window" in r.stderr.decode()


def test_cli_y4m_to_png_folder_and_png_folder_to_y4m(net3, tmp_path):
    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    n, h, w, sc = 9, 12, 14, (2.5, 3.0)
    frames = _i420(n, h, w, seed=13)
    src, dst, ckpt = tmp_path / "lr.y4m", tmp_path / "sr", tmp_path / "net.pth"
    src.write_bytes(_y4m_bytes(frames, h, w))
    sio.save_network(net3, str(ckpt))
    assert main(["-i", str(src), "-o", str(dst), "--scale", "2.5", "3", "--checkpoint", str(ckpt), "--chunk", "4"]) == 0
    names = [f"{i:08d}.png" for i in range(n)]
    assert sorted(os.listdir(dst)) == names
    ref = net3.upscale_video(_rgb_of(frames, h, w), scale=sc, out="uint8").cpu().numpy()        # today's uint8 RGB path on the converted frames
    for i, nm in enumerate(names):
        assert np.array_equal(np.asarray(Image.open(dst / nm)), ref[i]), nm
    # the other mix: the PNGs just written -> Y4M at --fps
    out = tmp_path / "again.y4m"
    assert main(["-i", str(dst), "-o", str(out), "--scale", "2", "--checkpoint", str(ckpt), "--fps", "24000:1001"]) == 0
    H, W = ref.shape[1:3]
    sr = net3.upscale_video(torch.from_numpy(ref), scale=2, out="i420").cpu().numpy()
    f = io.BytesIO()
    y4m.Y4MWriter(f, 2 * W, 2 * H, (24000, 1001), "p", (0, 0)).write(sr)
    assert out.read_bytes() == f.getvalue()
