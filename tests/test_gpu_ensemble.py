"""The self-ensemble on the GPU: the ensemble gather against torch flips / transposes of savsr_video_gather_*, the merge against the
torch restatement (fp32 bitwise; uint8 bitwise against savsr_video_quantize_u8 of it), SAVSR.forward with the switch on against the
restatement built from forward_many per variant (bitwise) and against the CPU oracle, upscale_video / VideoUpscaler / the CLI with the
switch on, and the num_in_ch = 1 and fp16 forms."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from PIL import Image

from savsr_amd.harness import window_indices
from savsr_amd.packing import get_hw
from savsr_amd.utils import synth
from tests.ensemble_cases import fwd_t, merge_t, variant_scale

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _lib():
    from savsr_amd import _lib as L
    return L.load()


def _idx(lst):
    return (C.c_int32 * len(lst))(*lst)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _net(seed=3, **cfg):
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR(**cfg)
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=seed), strict=True)
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def net3():
    return _net()


def _restated(net, clip, sc):
    """The ensemble of one clip [T, c, h, w] (device) from single passes: forward_many per variant, merged by the torch restatement."""
    on = net.self_ensemble
    net.set_self_ensemble(False)
    try:
        outs = [net.forward_many([fwd_t(clip, k)], [variant_scale(k, sc)])[0] for k in range(8)]
    finally:
        net.set_self_ensemble(on)
    return merge_t(outs)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("h,w", [(7, 9), (33, 40), (5, 70)])
def test_gather_bitwise(c, h, w):
    lib = _lib()
    n, T = 6, 5
    rng = np.random.RandomState(c * 100 + h * 7 + w)
    u8 = torch.from_numpy(rng.randint(0, 256, size=(n, h, w, c), dtype=np.uint8)).to(DEV)
    f32 = torch.from_numpy(rng.uniform(-1, 2, size=(n, c, h, w)).astype(np.float32)).to(DEV)
    idx = [int(v) for v in rng.randint(0, n, size=2 * T)]
    base_u8 = torch.empty(2 * T, c, h, w, device=DEV)
    base_f32 = torch.empty(2 * T, c, h, w, device=DEV)
    assert lib.savsr_video_gather_u8(u8.data_ptr(), n, c, h, w, _idx(idx), len(idx), base_u8.data_ptr(), _st()) == 0
    assert lib.savsr_video_gather_f32(f32.data_ptr(), n, c, h, w, _idx(idx), len(idx), base_f32.data_ptr(), _st()) == 0
    for k in range(8):
        shape = (2 * T, c, w, h) if k >> 2 else (2 * T, c, h, w)
        for src, base, fn in ((u8, base_u8, lib.savsr_ensemble_gather_u8), (f32, base_f32, lib.savsr_ensemble_gather_f32)):
            out = torch.full((int(np.prod(shape)) + 64,), 7.0, device=DEV)
            assert fn(src.data_ptr(), n, c, h, w, _idx(idx), len(idx), k, out.data_ptr(), _st()) == 0
            torch.cuda.synchronize()
            got = out[: int(np.prod(shape))].view(shape)
            assert torch.equal(got, fwd_t(base, k)), (k, src.dtype)
            assert bool((out[int(np.prod(shape)):] == 7.0).all())       # nothing written past the slots


@pytest.mark.parametrize("c,H,W", [(3, 37, 45), (1, 64, 96), (3, 17, 20), (2, 8, 8), (3, 100, 132), (1, 5, 3)])
def test_merge_bitwise(c, H, W):
    lib = _lib()
    rng = np.random.RandomState(c * 1000 + H + W)
    outs = []
    for k in range(8):                   # separate tensors, allocated out of order: offsets of both signs from the lowest pointer
        shape = (c, W, H) if k >> 2 else (c, H, W)
        outs.append(torch.from_numpy(rng.uniform(-0.3, 1.3, size=shape).astype(np.float32)).to(DEV))
    ptrs = [o.data_ptr() for o in outs]
    base = ptrs[3]
    offs = (C.c_int64 * 8)(*[(p - base) // 4 for p in ptrs])
    ref = merge_t(outs)
    got = torch.full((c * H * W + 64,), 5.0, device=DEV)
    assert lib.savsr_ensemble_merge(base, offs, c, H, W, 0, got.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(got[: c * H * W].view(c, H, W), ref)
    assert bool((got[c * H * W:] == 5.0).all())
    q_ref = torch.empty(H * W * c, dtype=torch.uint8, device=DEV)
    assert lib.savsr_video_quantize_u8(ref.data_ptr(), 1, c, H, W, q_ref.data_ptr(), _st()) == 0
    q = torch.full((H * W * c + 64,), 9, dtype=torch.uint8, device=DEV)
    assert lib.savsr_ensemble_merge(base, offs, c, H, W, 1, q.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(q[: H * W * c], q_ref)
    assert bool((q[H * W * c:] == 9).all())


@pytest.mark.parametrize("b,h,w,sc", [(1, 12, 17, (3.5, 2)), (2, 16, 20, (2, 3)), (1, 240, 300, (1.5, 1.2))])
def test_forward_bitwise_against_restatement(net3, b, h, w, sc):
    """Asymmetric scales, an odd width, two clips in one call, and a frame above SAVSR_CLIP_BATCH_MAX_PX (one clip per launch unit)."""
    lq = synth.synth_clip(7, 3, h, w, seed=h + w, batch=b).to(DEV)
    net3.set_scale(sc)
    net3.set_self_ensemble(True)
    try:
        out = net3(lq)
        many = net3.forward_many([lq[i] for i in range(b)], [sc] * b)
    finally:
        net3.set_self_ensemble(False)
    assert out.shape == (b, 3) + get_hw(h, w, sc)
    for i in range(b):
        ref = _restated(net3, lq[i], sc)
        assert torch.equal(out[i], ref), i
        assert torch.equal(many[i], ref), i
    single = net3(lq)                                          # the switch off: a single pass again
    assert not torch.equal(single[0], out[0])


def test_ensemble_against_oracle():
    """The CPU oracle on the 8 torch-transformed clips, each at its own scale, merged the same way: catches a missing scale swap."""
    from oracle import savsr_oracle as O
    sd = synth.synth_state_dict(seed=0)
    net = _net(seed=0)
    sc = (3.5, 2)
    lq = synth.synth_clip(7, 3, 10, 13, seed=4)
    net.set_scale(sc)
    net.set_self_ensemble(True)
    out = net(lq.to(DEV)).cpu()
    with torch.no_grad():
        outs = [O.forward(sd, fwd_t(lq, k), variant_scale(k, sc))[0] for k in range(8)]
    ref = merge_t(outs)
    assert out.shape[1:] == ref.shape
    assert float((out[0] - ref).abs().max()) < 5e-5


def _video_u8(n, h, w, c=3, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=(n, h, w, c), dtype=np.uint8)


def test_upscale_video_and_upscaler(net3):
    from savsr_amd import VideoUpscaler
    n, h, w, sc = 9, 11, 14, (2.5, 2)
    u8 = torch.from_numpy(_video_u8(n, h, w, seed=21))
    net3.set_self_ensemble(True)
    try:
        q = net3.upscale_video(u8, scale=sc, out="uint8")
        f = net3.upscale_video(u8.to(DEV), scale=sc)
        frames = torch.from_numpy(np.ascontiguousarray(u8.numpy().transpose(0, 3, 1, 2).astype(np.float32) / 255.0)).to(DEV)
        for i in range(n):
            win = frames[window_indices(i, n, 7, "reflection")]
            net3.set_scale(sc)
            ref = net3(win[None].contiguous())[0]
            assert torch.equal(f[i], ref), i
        lib = _lib()
        H, W = f.shape[2:]
        q_ref = torch.empty(n, H, W, 3, dtype=torch.uint8, device=DEV)
        assert lib.savsr_video_quantize_u8(f.data_ptr(), n, 3, H, W, q_ref.data_ptr(), _st()) == 0
        assert torch.equal(q, q_ref)
        for chunk in (2, 5):
            up = VideoUpscaler(net3, sc, out="uint8")
            net3.set_self_ensemble(False)          # read at construction: a later change does not reach it
            got = torch.cat([up.push(u8[a:a + chunk]) for a in range(0, n, chunk)] + [up.finish()], 0)
            net3.set_self_ensemble(True)
            assert torch.equal(got, q), chunk
    finally:
        net3.set_self_ensemble(False)


def test_cli_self_ensemble(net3, tmp_path):
    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    n, h, w = 8, 10, 12
    u8 = _video_u8(n, h, w, seed=31)
    src, dst = tmp_path / "lr", tmp_path / "sr"
    src.mkdir()
    names = [f"f{i:02d}.png" for i in range(n)]
    for i, nm in enumerate(names):
        Image.fromarray(u8[i]).save(src / nm)
    ckpt = tmp_path / "net.pth"
    sio.save_network(net3, str(ckpt))
    assert main(["-i", str(src), "-o", str(dst), "--scale", "2", "3.5", "--checkpoint", str(ckpt), "--chunk", "3", "--self-ensemble"]) == 0
    net3.set_self_ensemble(True)
    try:
        ref = net3.upscale_video(torch.from_numpy(u8), scale=(2, 3.5), out="uint8").cpu().numpy()
    finally:
        net3.set_self_ensemble(False)
    for i, nm in enumerate(names):
        assert np.array_equal(np.asarray(Image.open(dst / nm)), ref[i]), nm


def test_num_in_ch_1_and_fp16():
    net1 = _net(num_in_ch=1, num_feat=32)
    net1.set_scale((2, 3))
    net1.set_self_ensemble(True)
    lq = synth.synth_clip(7, 1, 9, 12, seed=8).to(DEV)
    out = net1(lq)
    assert out.shape == (1, 1, 18, 36) and bool(torch.isfinite(out).all())
    assert torch.equal(out[0], _restated(net1, lq[0], (2, 3)))
    net = _net()
    net.set_precision("fp16")
    net.set_scale((3, 2.5))
    net.set_self_ensemble(True)
    lq3 = synth.synth_clip(7, 3, 12, 10, seed=9).to(DEV)
    o16 = net(lq3)
    assert o16.shape == (1, 3, 36, 25) and bool(torch.isfinite(o16).all())
    net.set_precision("fp32")
    o32 = net(lq3)
    assert float((o16 - o32).abs().max()) < 2e-2
