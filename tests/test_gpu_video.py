"""The sequence path on the GPU: the window gather (savsr_video_gather_u8 / _f32) and the quantisation (savsr_video_quantize_u8) bit for
bit against numpy / metrics.tensor2img, SAVSR.upscale_video against the REFERENCE's per-window outputs (tests/golden/video_outputs.npz),
bitwise against forward_many on hand-gathered windows, VideoUpscaler against upscale_video for any chunking, and the CLI end to end."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from savsr_amd.harness import window_indices
from savsr_amd.metrics import tensor2img
from savsr_amd.utils import synth
from tests.video_cases import PADDINGS, VIDEO_CASES, VIDEO_SEED, WEIGHT_SEED

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def _lib():
    from savsr_amd import _lib as L
    return L.load()


def _idx(lst):
    import ctypes as C
    return (C.c_int32 * len(lst))(*lst)


def _net(seed=WEIGHT_SEED, **cfg):
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR(**cfg)
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=seed), strict=True)
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def net3():
    return _net()


@pytest.fixture(scope="module")
def vgold():
    return np.load(os.path.join(ROOT, "tests", "golden", "video_outputs.npz"))


def _video_u8(n, h, w, c=3, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=(n, h, w, c), dtype=np.uint8)


@pytest.mark.parametrize("c", [1, 2, 3])
@pytest.mark.parametrize("h,w", [(7, 9), (8, 12), (5, 3)])
@pytest.mark.parametrize("nb,nf", [(1, 5), (2, 7), (3, 9), (4, 7)])
def test_gather_u8_bitwise(c, h, w, nb, nf):
    lib = _lib()
    n = nf + 3
    frames = _video_u8(n, h, w, c, seed=c * 100 + h + nb)
    rng = np.random.RandomState(nb * 10 + nf)
    idx = [int(v) for v in rng.randint(0, n, size=nb * nf)]
    ref = (frames.astype(np.float32) / 255.0)[idx].transpose(0, 3, 1, 2)                  # read_img_seq / img2tensor
    total = nb * nf * c * h * w
    out = torch.full((total + 64,), float("nan"), device=DEV)                          # poisoned: everything written, nothing beyond
    fd = torch.from_numpy(frames).to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.savsr_video_gather_u8(fd.data_ptr(), n, c, h, w, _idx(idx), len(idx), out.data_ptr(), st) == 0
    torch.cuda.synchronize()
    got = out[:total].cpu().numpy().reshape(nb * nf, c, h, w)
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(ref).view(np.uint32))
    assert bool(torch.isnan(out[total:]).all())
    # the fp32 planar source: a copy of the named frames
    ff = torch.from_numpy(np.ascontiguousarray(frames.transpose(0, 3, 1, 2).astype(np.float32) / 255.0)).to(DEV)
    out2 = torch.full((total + 64,), float("nan"), device=DEV)
    assert lib.savsr_video_gather_f32(ff.data_ptr(), n, c, h, w, _idx(idx), len(idx), out2.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out2[:total].cpu(), out[:total].cpu())
    assert bool(torch.isnan(out2[total:]).all())


def test_gather_covers_every_byte_value():
    lib = _lib()
    frames = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1)
    out = torch.empty(256, device=DEV)
    fd = torch.from_numpy(frames).to(DEV)
    assert lib.savsr_video_gather_u8(fd.data_ptr(), 1, 1, 16, 16, _idx([0]), 1, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), (np.arange(256, dtype=np.uint8).astype(np.float32) / 255.0).view(np.uint32))


def test_gather_refuses_bad_indices():
    lib = _lib()
    fd = torch.zeros(2 * 4 * 4 * 3, dtype=torch.uint8, device=DEV)
    out = torch.zeros(64 * 48, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.savsr_video_gather_u8(fd.data_ptr(), 2, 3, 4, 4, _idx([0, 2]), 2, out.data_ptr(), st) < 0        # frame 2 of 2
    assert lib.savsr_video_gather_u8(fd.data_ptr(), 2, 3, 4, 4, _idx([-1]), 1, out.data_ptr(), st) < 0
    assert lib.savsr_video_gather_u8(fd.data_ptr(), 2, 3, 4, 4, _idx([0] * 65), 65, out.data_ptr(), st) < 0     # > SAVSR_VIDEO_MAX_SLOTS
    assert lib.savsr_video_gather_u8(fd.data_ptr(), 2, 4, 4, 4, _idx([0]), 1, out.data_ptr(), st) < 0           # c = 4
    assert b"video_gather_u8" in lib.savsr_last_error()


def _quant_ref(x: torch.Tensor) -> np.ndarray:
    return np.stack([tensor2img(x[i], rgb2bgr=False).reshape(x.shape[2], x.shape[3], x.shape[1]) for i in range(x.shape[0])], 0)


@pytest.mark.parametrize("n,c,H,W", [(2, 3, 16, 24), (3, 1, 8, 8), (1, 2, 4, 12), (2, 3, 7, 9), (1, 1, 5, 5), (1, 3, 720, 1280)])
def test_quantize_u8_bitwise(n, c, H, W):
    lib = _lib()
    rng = np.random.RandomState(n * 7 + c + H)
    x = rng.uniform(-0.25, 1.25, size=(n, c, H, W)).astype(np.float32)
    flat = x.reshape(-1)
    k = np.arange(min(flat.size, 4 * 256)) % 256
    flat[: k.size] = ((k + 0.5) / 255.0).astype(np.float32)                              # ties at x 255 (and their float neighbours)
    flat[k.size: 2 * k.size] = np.nextafter(flat[: k.size], np.float32(2.0))[: flat[k.size: 2 * k.size].size]
    xt = torch.from_numpy(x)
    ref = _quant_ref(xt)
    total = n * c * H * W
    out = torch.full((total + 64,), 7, dtype=torch.uint8, device=DEV)
    xd = xt.to(DEV)
    assert lib.savsr_video_quantize_u8(xd.data_ptr(), n, c, H, W, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    got = out[:total].cpu().numpy().reshape(n, H, W, c)
    assert np.array_equal(got, ref)
    assert bool((out[total:] == 7).all())


@pytest.mark.parametrize("name,cfg,n,h,w,sc,padding", VIDEO_CASES)
def test_upscale_video_vs_reference_golden(vgold, name, cfg, n, h, w, sc, padding):
    net = _net(**cfg)
    video = synth.synth_clip(n, cfg.get("num_in_ch", 3), h, w, seed=VIDEO_SEED)[0].to(DEV)
    sr = net.upscale_video(video, scale=sc, padding=padding)
    gold = torch.from_numpy(vgold[f"{name}/sr"])
    assert sr.shape == gold.shape
    assert float((sr.cpu() - gold).abs().max()) < 5e-5


def test_upscale_video_equals_forward_many_on_gathered_windows(net3):
    """23 frames of 16 x 20: 8 launch units of up to 3 windows over the streams; every frame bit for bit forward_many's on its window,
    uint8 output = tensor2img of the fp32 output, uint8 input = fp32 input fed u8 / 255."""
    n, h, w, sc = 23, 16, 20, (2.5, 2.0)
    u8 = _video_u8(n, h, w, seed=23)
    f32 = torch.from_numpy(np.ascontiguousarray(u8.transpose(0, 3, 1, 2).astype(np.float32) / 255.0)).to(DEV)
    sr = net3.upscale_video(f32, scale=sc)
    clips = [f32[window_indices(i, n, 7, "reflection")] for i in range(n)]
    ref = net3.forward_many(clips, [sc] * n)
    for i in range(n):
        assert torch.equal(sr[i], ref[i]), i
    sr_u = net3.upscale_video(torch.from_numpy(u8), scale=sc)          # host uint8 in
    assert torch.equal(sr_u, sr)
    q = net3.upscale_video(torch.from_numpy(u8).to(DEV), scale=sc, out="uint8")
    assert q.dtype == torch.uint8 and q.shape == (n,) + sr.shape[2:] + (3,)
    assert np.array_equal(q.cpu().numpy(), _quant_ref(sr.cpu()))


@pytest.mark.parametrize("padding", PADDINGS)
def test_video_upscaler_any_chunking_is_bitwise(net3, padding):
    from savsr_amd import VideoUpscaler
    n, h, w = 13, 10, 12
    u8 = torch.from_numpy(_video_u8(n, h, w, seed=5))
    whole = net3.upscale_video(u8, scale=3, padding=padding)
    for chunk in (1, 3, 7, n):
        up = VideoUpscaler(net3, 3, padding)
        parts = [up.push(u8[a:a + chunk]) for a in range(0, n, chunk)]
        parts.append(up.finish())
        got = torch.cat(parts, 0)
        assert torch.equal(got, whole), (padding, chunk)
    up = VideoUpscaler(net3, 3, padding, out="uint8")
    got = torch.cat([up.push(u8[a:a + 4].to(DEV)) for a in range(0, n, 4)] + [up.finish()], 0)
    assert torch.equal(got, net3.upscale_video(u8, scale=3, padding=padding, out="uint8"))


def test_video_upscaler_memory_stays_flat(net3):
    from savsr_amd import VideoUpscaler
    u8 = torch.from_numpy(_video_u8(200, 64, 64, seed=9))
    up = VideoUpscaler(net3, 2, "reflection", out="uint8")
    seen, n_out = [], 0
    for a in range(0, 200, 5):
        n_out += up.push(u8[a:a + 5]).shape[0]
        torch.cuda.synchronize()
        if a >= 50:                                            # after warm-up: every (unit size, stream) graph has been captured
            seen.append(torch.cuda.memory_allocated(DEV))
    n_out += up.finish().shape[0]
    assert n_out == 200
    assert max(seen) - min(seen) <= 1 << 20, (min(seen), max(seen))      # 1 MiB: less than the 12 frames the upscaler holds at 64 x 64 x 4 floats


def test_cli_writes_what_upscale_video_returns(net3, tmp_path):
    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    n, h, w = 9, 12, 14
    u8 = _video_u8(n, h, w, seed=11)
    src, dst = tmp_path / "lr", tmp_path / "sr"
    src.mkdir()
    names = [f"im{i:03d}.png" for i in range(n)]
    for i, nm in enumerate(names):
        Image.fromarray(u8[i]).save(src / nm)
    ckpt = tmp_path / "net.pth"
    sio.save_network(net3, str(ckpt))
    assert main(["-i", str(src), "-o", str(dst), "--scale", "2.5", "3", "--checkpoint", str(ckpt), "--chunk", "4"]) == 0
    assert sorted(os.listdir(dst)) == names
    ref = net3.upscale_video(torch.from_numpy(u8), scale=(2.5, 3), out="uint8").cpu().numpy()
    for i, nm in enumerate(names):
        assert np.array_equal(np.asarray(Image.open(dst / nm)), ref[i]), nm
