"""Luma-only checkpoints on the GPU: savsr_video_gather_luma / savsr_video_quantize_luma / savsr_video_resample_chroma bit for bit against
their numpy restatement (savsr_amd/yuv.py, which tests/test_luma.py pins); then chroma_filter="bicubic" and "y400" of SAVSR.upscale_video,
VideoUpscaler, cuts=, the self-ensemble, fp16 and the CLI against the composition by hand: the network's luma on the Y planes as
[N, h, w, 1] frames -> yuv.luma_only_frames."""
import ctypes as C

import numpy as np
import pytest
import torch

from savsr_amd import yuv
from savsr_amd.packing import get_hw
from savsr_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
E_ARG, E_ALIGN = -1, -2
LUMA_SIZES = [(5, 3, 0), (6, 8, 0), (18, 20, 0), (181, 319, 0), (6, 8, 1)]        # (h, w, samples off alignment); 6 x 8 off by one: scalar form
IDX = [2, 0, 0, 1, 2, 2, 0]                                                        # repeated and out of order
SCALES = [(1, 1), (2, 2), (2.7, 3.3), (1.5, 4), (4, 4)]
RESAMPLE_SIZES = [(5, 3), (6, 8), (13, 17), (40, 72)]
DEPTH_PAIRS = [(8, 8), (8, 10), (10, 8), (12, 12)]
SITING_PAIRS = [("left", "left"), ("topleft", "topleft"), (None, None), ("centre", "left"), ("left", "topleft"), ("topleft", "centre")]


def _lib():
    from savsr_amd import _lib as L
    return L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _idx(idx):
    return (C.c_int32 * len(idx))(*idx)


def _samples(shape, depth, seed):
    """Random codes over the whole range; at 10 / 12 bits some lie above 2^depth - 1, the first one always."""
    rng = np.random.RandomState(seed)
    if depth == 8:
        return rng.randint(0, 256, size=shape).astype(np.uint8)
    s = rng.randint(0, 1 << depth, size=shape)
    over = rng.uniform(size=shape) < 0.1
    s[over] = rng.randint(1 << depth, 1 << 16, size=int(over.sum()))
    s.reshape(-1)[0] = 0xffff
    return s.astype("<u2")


def _device_bytes(host_u8: np.ndarray, boff: int):
    """The bytes on the device, boff bytes off an allocation's (16-byte aligned) start, with slack behind."""
    raw = torch.zeros(host_u8.size + 64, dtype=torch.uint8, device=DEV)
    raw[boff:boff + host_u8.size] = torch.from_numpy(host_u8.reshape(-1)).to(DEV)
    assert raw.data_ptr() % 16 == 0
    return raw, raw.data_ptr() + boff


def _valid(siting, chroma):
    return not (siting == "topleft" and chroma == "422")


# ---------------------------------------------------------------------------------------------------------------- gather and quantise
@pytest.mark.parametrize("depth", [8, 10, 12])
@pytest.mark.parametrize("h,w,off", LUMA_SIZES)
def test_gather_luma_bitwise(h, w, off, depth):
    """The Y plane inside an I420 frame (a stride larger than the plane), an index list with repeats, samples above 2^depth - 1."""
    s = 1 if depth == 8 else 2
    fb = yuv.frame_bytes(h, w, depth, "420")
    n = 3
    frames = _samples((n, fb // s), depth, seed=h * 7 + w + depth)
    raw, ptr = _device_bytes(frames.view(np.uint8), off * s)
    out = torch.full((len(IDX) * h * w + 64,), float("nan"), device=DEV)
    rc = _lib().savsr_video_gather_luma(ptr, n, fb, h, w, depth, _idx(IDX), len(IDX), out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    got = out.cpu().numpy()
    ref = yuv.luma_to_unit(frames[:, :h * w], depth)[IDX].reshape(-1)
    assert got[:ref.size].view(np.uint32).tolist() == ref.view(np.uint32).tolist()
    assert np.isnan(got[ref.size:]).all()
    if depth == 8:          # savsr_video_gather_u8's value
        assert np.array_equal(ref, (frames[:, :h * w].astype(np.float32) / np.float32(255.0))[IDX].reshape(-1))


@pytest.mark.parametrize("depth", [8, 10, 12])
@pytest.mark.parametrize("H,W,off", LUMA_SIZES)
def test_quantize_luma_bitwise(H, W, off, depth):
    """Into the Y plane of I420 frames: the chroma bytes behind it stay as they were."""
    s = 1 if depth == 8 else 2
    fb = yuv.frame_bytes(H, W, depth, "420")
    n = 2
    rng = np.random.RandomState(H + 3 * W + depth)
    x = rng.uniform(-0.2, 1.2, size=(n, 1, H, W)).astype(np.float32)
    k = 255 << (depth - 8)
    x.reshape(-1)[:8] = [np.nan, np.inf, -np.inf, 0.5 / k, 1.5 / k, 2.5 / k, 1.0, -0.0][:min(8, x.size)]          # ties: half to even
    xd = torch.from_numpy(x).to(DEV)
    raw = torch.full((n * fb + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    rc = _lib().savsr_video_quantize_luma(xd.data_ptr(), n, H, W, depth, raw.data_ptr() + off * s, fb, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    got = raw.cpu().numpy()
    ref = yuv.unit_to_luma(x[:, 0], depth)
    body = got[off * s:off * s + n * fb].reshape(n, fb)
    assert np.array_equal(body[:, :H * W * s], ref.astype(np.uint8 if depth == 8 else "<u2").reshape(n, -1).view(np.uint8))
    assert (body[:, H * W * s:] == 0xAB).all() and (got[:off * s] == 0xAB).all() and (got[off * s + n * fb:] == 0xAB).all()


@pytest.mark.parametrize("depth", [8, 10])
def test_luma_frame_stride_off_the_vector_alignment(depth):
    """w % 4 == 0 and aligned pointers, but a frame stride that is no multiple of 4 (8 at 16 bits) bytes: the host takes the scalar form,
    since only frame 0 would keep the alignment of a 4-sample access.  Both entries, frames 1 and 2 included."""
    h, w, n = 6, 8, 3
    s = 1 if depth == 8 else 2
    fb = (h * w + 1) * s                                  # 49 or 98 bytes
    frames = _samples((n, fb // s), depth, seed=depth)
    raw, ptr = _device_bytes(frames.view(np.uint8), 0)
    out = torch.full((n * h * w + 16,), float("nan"), device=DEV)
    assert _lib().savsr_video_gather_luma(ptr, n, fb, h, w, depth, _idx([2, 1, 0]), 3, out.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    ref = yuv.luma_to_unit(frames[:, :h * w], depth)[[2, 1, 0]].reshape(-1)
    got = out.cpu().numpy()
    assert got[:ref.size].view(np.uint32).tolist() == ref.view(np.uint32).tolist() and np.isnan(got[ref.size:]).all()
    x = np.random.RandomState(depth).uniform(-0.1, 1.1, size=(n, 1, h, w)).astype(np.float32)
    dst = torch.full((n * fb + 16,), 0xAB, dtype=torch.uint8, device=DEV)
    assert _lib().savsr_video_quantize_luma(torch.from_numpy(x).to(DEV).data_ptr(), n, h, w, depth, dst.data_ptr(), fb, _stream()) == 0
    torch.cuda.synchronize()
    body = dst.cpu().numpy()[:n * fb].reshape(n, fb)
    assert np.array_equal(body[:, :h * w * s], yuv.unit_to_luma(x[:, 0], depth).astype(np.uint8 if depth == 8 else "<u2").reshape(n, -1).view(np.uint8))
    assert (body[:, h * w * s:] == 0xAB).all() and (dst.cpu().numpy()[n * fb:] == 0xAB).all()


def test_luma_entries_refuse_before_the_device():
    lib = _lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    f = torch.zeros(1024, device=DEV)
    p, st = buf.data_ptr(), _stream()

    def err():
        return lib.savsr_last_error().decode()
    assert lib.savsr_video_gather_luma(p, 2, 48, 4, 4, 9, _idx([0]), 1, f.data_ptr(), st) == E_ARG and "depth" in err()
    assert lib.savsr_video_gather_luma(p, 2, 15, 4, 4, 8, _idx([0]), 1, f.data_ptr(), st) == E_ARG and "frame_bytes" in err()
    assert lib.savsr_video_gather_luma(p, 2, 48, 4, 4, 8, _idx([2]), 1, f.data_ptr(), st) == E_ARG and "frame 2 of 2" in err()
    assert lib.savsr_video_gather_luma(p, 2, 48, 4, 4, 8, _idx([0] * 65), 65, f.data_ptr(), st) == E_ARG
    assert lib.savsr_video_gather_luma(p + 1, 2, 48, 4, 4, 10, _idx([0]), 1, f.data_ptr(), st) == E_ALIGN and "2-byte" in err()
    assert lib.savsr_video_gather_luma(p, 2, 49, 4, 4, 12, _idx([0]), 1, f.data_ptr(), st) == E_ALIGN
    assert lib.savsr_video_gather_luma(0, 2, 48, 4, 4, 8, _idx([0]), 1, f.data_ptr(), st) == E_ARG and "null" in err()
    assert lib.savsr_video_quantize_luma(f.data_ptr(), 1, 4, 4, 11, p, 48, st) == E_ARG and "depth" in err()
    assert lib.savsr_video_quantize_luma(f.data_ptr(), 1, 4, 4, 8, p, 15, st) == E_ARG and "out_frame_bytes" in err()
    assert lib.savsr_video_quantize_luma(f.data_ptr(), 1, 4, 4, 10, p + 1, 48, st) == E_ALIGN
    assert lib.savsr_video_quantize_luma(f.data_ptr(), 0, 4, 4, 8, p, 48, st) == E_ARG
    t = torch.zeros(64, dtype=torch.int32, device=DEV)
    wt = torch.zeros(64, device=DEV)

    def resample(src=p, n=1, sfb=24, soff=16, ch=2, cw=2, d=8, dst=p + 1024, dfb=96, doff=64, cH=4, cW=4, D=8, ty=1, tx=1):
        return lib.savsr_video_resample_chroma(src, n, sfb, soff, ch, cw, d, dst, dfb, doff, cH, cW, D, t.data_ptr(), t.data_ptr(), wt.data_ptr(), ty,
                                               t.data_ptr(), t.data_ptr(), wt.data_ptr(), tx, st)
    assert resample(soff=21) == E_ARG and "source plane" in err()
    assert resample(doff=81) == E_ARG and "destination plane" in err()
    assert resample(d=9) == E_ARG and "depth" in err()
    assert resample(ty=0) == E_ARG and "taps" in err()
    assert resample(src=0) == E_ARG
    assert resample(d=10, sfb=48, soff=17) == E_ALIGN and "source" in err()
    assert resample(D=12, dfb=192, doff=64, dst=p + 1025) == E_ALIGN and "destination" in err()
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0          # nothing was written


# ---------------------------------------------------------------------------------------------------------------- the resampler
def _resample_gpu(plane, d, D, tables, cH, cW, n_pad=5):
    """One plane of n frames through savsr_video_resample_chroma, the plane at an offset inside a larger frame on either side; the
    destination is poisoned: the plane is written, nothing beyond."""
    (ym, ys, wy), (xm, xs, wx) = tables
    n, ch, cw = plane.shape
    si, so = (1 if d == 8 else 2), (1 if D == 8 else 2)
    soff, doff = 6 * si, 10 * so
    sfb, dfb = soff + ch * cw * si + n_pad * si, doff + cH * cW * so + 3 * so
    src = np.zeros((n, sfb), np.uint8)
    src[:, soff:soff + ch * cw * si] = plane.astype(np.uint8 if d == 8 else "<u2").reshape(n, -1).view(np.uint8)
    sd = torch.from_numpy(src).to(DEV)
    dd = torch.full((n, dfb), 0xCD, dtype=torch.uint8, device=DEV)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (ym, ys, wy, xm, xs, wx)]
    rc = _lib().savsr_video_resample_chroma(sd.data_ptr(), n, sfb, soff, ch, cw, d, dd.data_ptr(), dfb, doff, cH, cW, D, dev[0].data_ptr(),
                                            dev[1].data_ptr(), dev[2].data_ptr(), wy.shape[1], dev[3].data_ptr(), dev[4].data_ptr(),
                                            dev[5].data_ptr(), wx.shape[1], _stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib().savsr_last_error()
    got = dd.cpu().numpy()
    assert (got[:, :doff] == 0xCD).all() and (got[:, doff + cH * cW * so:] == 0xCD).all()
    body = np.ascontiguousarray(got[:, doff:doff + cH * cW * so])
    return (body if D == 8 else body.view("<u2")).reshape(n, cH, cW)


def _check_resample(h, w, scale, lay, out_lay, sit, out_sit, d, D, seed=0):
    H, W = get_hw(h, w, scale)
    tables = yuv.chroma_tables(h, w, H, W, lay, out_lay, sit, out_sit)
    ch, cw = yuv.chroma_hw(h, w, lay)
    cH, cW = yuv.chroma_hw(H, W, out_lay)
    plane = _samples((2, ch, cw), d, seed + h + w)
    ref = yuv.resample_chroma(plane, tables[0], tables[1], d, D)
    got = _resample_gpu(plane, d, D, tables, cH, cW)
    assert np.array_equal(got, ref), (h, w, scale, lay, out_lay, sit, out_sit, d, D, int((got != ref).sum()))


@pytest.mark.parametrize("h,w", RESAMPLE_SIZES)
def test_resample_chroma_bitwise_sizes_scales_layouts(h, w):
    """Every scale and every in / out layout pair at this size; the siting and depth pairs cycle so that each is met at every size."""
    k = 0
    for scale in SCALES:
        for lay in yuv.CHROMAS:
            for out_lay in yuv.CHROMAS:
                sit, out_sit = SITING_PAIRS[k % len(SITING_PAIRS)]
                d, D = DEPTH_PAIRS[(k // 2) % len(DEPTH_PAIRS)]
                k += 1
                sit = sit if _valid(sit, lay) else "left"
                out_sit = out_sit if _valid(out_sit, out_lay) else "left"
                _check_resample(h, w, scale, lay, out_lay, sit, out_sit, d, D, seed=k)


@pytest.mark.parametrize("d,D", DEPTH_PAIRS)
def test_resample_chroma_bitwise_sitings_depths(d, D):
    """Every layout pair with both cosited sitings (and a mixed pair) at every depth pair, at 13 x 17 x (2.7, 3.3)."""
    for lay in yuv.CHROMAS:
        for out_lay in yuv.CHROMAS:
            for sit, out_sit in (("left", "left"), ("topleft", "topleft"), ("left", "centre")):
                if _valid(sit, lay) and _valid(out_sit, out_lay):
                    _check_resample(13, 17, (2.7, 3.3), lay, out_lay, sit, out_sit, d, D)


def test_resample_chroma_downscales_and_loops_over_lds_buffers():
    """4:4:4 in, 4:2:0 out at x 1.5 (rho = 4 / 3: 8 taps); and a tile whose 16 output rows need more than the 32 staged rows of one LDS
    buffer (4:4:4 -> 4:2:0 at x 0.5: rho = 4, 18 taps, 16 rows reach over ~80 input rows), which the kernel serves by looping."""
    _check_resample(13, 17, (1.5, 1.5), "444", "420", "left", "left", 8, 8)
    _check_resample(40, 72, (1.5, 1.5), "444", "420", None, "topleft", 10, 10)
    h, w = 160, 40
    tables = yuv.chroma_tables(h, w, 80, 20, "444", "420", None, None)
    assert tables[0][2].shape[1] >= 16 and int((tables[0][0][15] + tables[0][1][15]) - tables[0][0][0]) > 32
    plane = _samples((1, h, w), 8, 3)
    ref = yuv.resample_chroma(plane, tables[0], tables[1], 8, 8)
    assert np.array_equal(_resample_gpu(plane, 8, 8, tables, 40, 10), ref)


# ---------------------------------------------------------------------------------------------------------------- the public path
CFG = dict(num_in_ch=1, num_feat=32)
N, LH, LW, SC = 9, 12, 16, (2.5, 3)


@pytest.fixture(scope="module")
def net1():
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR(**CFG)
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=3), strict=True)
    return net.to(DEV).eval()


def _video(depth=8, chroma="420", seed=0):
    ns = yuv.frame_bytes(LH, LW, 8, chroma)
    s = np.random.RandomState(seed).randint(16 << (depth - 8), 236 << (depth - 8), size=(N, ns))
    return s.astype(np.uint8) if depth == 8 else s.astype("<u2").view(np.uint8)


@pytest.fixture(scope="module")
def ref8(net1):
    """The shared reference: the 8-bit I420 video, its Y planes through the network as [N, h, w, 1] frames (float and uint8)."""
    frames = _video()
    y = yuv.luma_plane(frames, LH, LW)
    y4 = torch.from_numpy(np.ascontiguousarray(y[..., None]))
    return frames, net1.upscale_video(y4, SC, out="float").cpu().numpy(), net1.upscale_video(y4, SC, out="uint8").cpu().numpy()


def _planes(out, H, W, depth=8, chroma="420"):
    return yuv.split_planes(out, H, W, depth, chroma)


def test_upscale_video_luma_i420(net1, ref8):
    frames, sr_f, sr_u8 = ref8
    H, W = get_hw(LH, LW, SC)
    out = net1.upscale_video(torch.from_numpy(frames), SC, out="i420", pixel_format="i420", size=(LH, LW), chroma_filter="bicubic").cpu().numpy()
    assert out.shape == (N, yuv.frame_bytes(H, W))
    y, u, v = _planes(out, H, W)
    assert np.array_equal(y, sr_u8[..., 0])
    ty, tx = yuv.chroma_tables(LH, LW, H, W, "420", "420")
    _, u0, v0 = yuv.split_planes(frames, LH, LW)
    assert np.array_equal(u, yuv.resample_chroma(u0, ty, tx)) and np.array_equal(v, yuv.resample_chroma(v0, ty, tx))
    assert np.array_equal(out, yuv.luma_only_frames(frames, LH, LW, sr_f))
    # the luma alone
    f = net1.upscale_video(torch.from_numpy(frames), SC, out="float", pixel_format="i420", size=(LH, LW), chroma_filter="bicubic")
    assert f.shape == (N, 1, H, W) and np.array_equal(f.cpu().numpy(), sr_f)
    q = net1.upscale_video(torch.from_numpy(frames), SC, out="uint8", pixel_format="i420", size=(LH, LW), chroma_filter="bicubic")
    assert q.shape == (N, H, W, 1) and np.array_equal(q.cpu().numpy(), sr_u8)
    # without the argument: the refusal as it was
    with pytest.raises(ValueError, match="I420 frames are colour frames, the network takes num_in_ch = 1"):
        net1.upscale_video(torch.from_numpy(frames), SC, pixel_format="i420", size=(LH, LW))


def test_upscale_video_luma_10_bits_layouts_sitings(net1):
    """10 bits in and out against unit_to_luma of the float result; 4:2:2 in, 4:4:4 out at 12 -> 8 bits with sitings."""
    H, W = get_hw(LH, LW, SC)
    frames = _video(10, "420", seed=1)
    t = torch.from_numpy(frames)
    kw = dict(pixel_format="i420", size=(LH, LW), depth=10, chroma_filter="bicubic")
    f = net1.upscale_video(t, SC, out="float", **kw).cpu().numpy()
    assert np.array_equal(f[:, 0], net1.upscale_video(torch.from_numpy(yuv.luma_to_unit(yuv.luma_plane(frames, LH, LW, 10), 10)[:, None]).to(DEV),
                                                      SC).cpu().numpy()[:, 0])
    out = net1.upscale_video(t, SC, out="i420", **kw).cpu().numpy()
    y, u, v = _planes(out, H, W, 10)
    assert np.array_equal(y, yuv.unit_to_luma(f[:, 0], 10))
    assert np.array_equal(out, yuv.luma_only_frames(frames, LH, LW, f, 10))
    frames = _video(12, "422", seed=2)
    kw = dict(pixel_format="i422", size=(LH, LW), depth=12, siting="left", chroma_filter="bicubic")
    f = net1.upscale_video(torch.from_numpy(frames), SC, out="float", **kw).cpu().numpy()
    out = net1.upscale_video(torch.from_numpy(frames), SC, out="i444", out_depth=8, **kw).cpu().numpy()
    assert np.array_equal(out, yuv.luma_only_frames(frames, LH, LW, f, 12, 8, "422", "444", "left", None))


def test_streaming_in_chunks_of_4(net1, ref8):
    from savsr_amd import VideoUpscaler
    frames, sr_f, _ = ref8
    up = VideoUpscaler(net1, SC, out="i420", pixel_format="i420", size=(LH, LW), chroma_filter="bicubic")
    parts = [up.push(torch.from_numpy(frames[a:a + 4])) for a in range(0, N, 4)] + [up.finish()]
    assert np.array_equal(torch.cat(parts, 0).cpu().numpy(), yuv.luma_only_frames(frames, LH, LW, sr_f))


def test_cuts(net1, ref8):
    frames = ref8[0]
    y4 = torch.from_numpy(np.ascontiguousarray(yuv.luma_plane(frames, LH, LW)[..., None]))
    sr = net1.upscale_video(y4, SC, cuts=[4]).cpu().numpy()
    out = net1.upscale_video(torch.from_numpy(frames), SC, out="i420", pixel_format="i420", size=(LH, LW), cuts=[4], chroma_filter="bicubic")
    assert np.array_equal(out.cpu().numpy(), yuv.luma_only_frames(frames, LH, LW, sr))


def test_self_ensemble(net1, ref8):
    frames = ref8[0]
    y4 = torch.from_numpy(np.ascontiguousarray(yuv.luma_plane(frames, LH, LW)[..., None]))
    net1.set_self_ensemble(True)
    try:
        sr = net1.upscale_video(y4, SC).cpu().numpy()
        out = net1.upscale_video(torch.from_numpy(frames), SC, out="i420", pixel_format="i420", size=(LH, LW), chroma_filter="bicubic")
    finally:
        net1.set_self_ensemble(False)
    assert not np.array_equal(sr, ref8[1])
    assert np.array_equal(out.cpu().numpy(), yuv.luma_only_frames(frames, LH, LW, sr))          # chroma never enters the ensemble


def test_fp16(net1, ref8):
    frames = ref8[0]
    y4 = torch.from_numpy(np.ascontiguousarray(yuv.luma_plane(frames, LH, LW)[..., None]))
    net1.set_precision("fp16")
    try:
        sr = net1.upscale_video(y4, SC).cpu().numpy()
        out = net1.upscale_video(torch.from_numpy(frames), SC, out="i420", pixel_format="i420", size=(LH, LW), chroma_filter="bicubic")
    finally:
        net1.set_precision("fp32")
    assert np.array_equal(out.cpu().numpy(), yuv.luma_only_frames(frames, LH, LW, sr))


def test_y400_in_and_out(net1, ref8):
    frames, sr_f, sr_u8 = ref8
    H, W = get_hw(LH, LW, SC)
    mono = np.ascontiguousarray(frames[:, :LH * LW])
    out = net1.upscale_video(torch.from_numpy(mono), SC, out="y400", pixel_format="y400", size=(LH, LW)).cpu().numpy()
    assert out.shape == (N, H * W) and np.array_equal(out.reshape(N, H, W), sr_u8[..., 0])
    # YUV in, y400 out drops the chroma; 8 -> 10 bits
    out10 = net1.upscale_video(torch.from_numpy(frames), SC, out="y400", pixel_format="i420", size=(LH, LW), out_depth=10,
                               chroma_filter="bicubic").cpu().numpy()
    assert np.array_equal(out10.view("<u2").reshape(N, H, W), yuv.unit_to_luma(sr_f[:, 0], 10))
    from savsr_amd import pair_sad
    from savsr_amd.scenes import pair_sad as pair_sad_spec
    assert pair_sad(torch.from_numpy(mono), "y400", (LH, LW)).cpu().tolist() == pair_sad_spec(mono, "y400", (LH, LW)).tolist()
    m12 = _samples((4, LH * LW), 12, 5).view(np.uint8)
    assert pair_sad(torch.from_numpy(m12), "y400", (LH, LW), 12).cpu().tolist() == pair_sad_spec(m12, "y400", (LH, LW), 12).tolist()


def _write_y4m(path, frames, w, h, chroma, siting=None):
    from savsr_amd.y4m import Y4MWriter
    with open(path, "wb") as f:
        Y4MWriter(f, w, h, chroma=chroma, siting=siting).write(frames)


def test_cli_y4m_colour_and_mono(net1, ref8, tmp_path):
    """.y4m -> .y4m through python -m savsr_amd.upscale's main() with a luma checkpoint from a YAML: a C420mpeg2 file with --chroma-filter
    bicubic --siting auto --out-siting same, and a Cmono file."""
    from savsr_amd import upscale
    from savsr_amd.y4m import Y4MReader
    frames, sr_f, sr_u8 = ref8
    H, W = get_hw(LH, LW, SC)
    ckpt = tmp_path / "luma.pth"
    torch.save({"params": {k: v.cpu() for k, v in net1.state_dict().items()}}, ckpt)
    opt = tmp_path / "luma.yml"
    opt.write_text(f"network_g:\n  type: SAVSR\n  num_in_ch: 1\n  num_feat: 32\npath:\n  pretrain_network_g: {ckpt}\n  strict_load_g: true\n")
    common = ["--scale", str(SC[0]), str(SC[1]), "--opt", str(opt), "--chunk", "4"]
    _write_y4m(tmp_path / "in.y4m", frames, LW, LH, "420", "left")
    assert upscale.main(["-i", str(tmp_path / "in.y4m"), "-o", str(tmp_path / "out.y4m"), "--chroma-filter", "bicubic", "--siting", "auto",
                         "--out-siting", "same"] + common) == 0
    with open(tmp_path / "out.y4m", "rb") as f:
        r = Y4MReader(f)
        assert (r.width, r.height, r.colorspace) == (W, H, "420mpeg2")
        got = np.concatenate(list(r.chunks(16)), 0)
    assert np.array_equal(got, yuv.luma_only_frames(frames, LH, LW, sr_f, siting="left", out_siting="left"))
    mono = np.ascontiguousarray(frames[:, :LH * LW])
    _write_y4m(tmp_path / "mono.y4m", mono, LW, LH, "400")
    assert upscale.main(["-i", str(tmp_path / "mono.y4m"), "-o", str(tmp_path / "mono_out.y4m")] + common) == 0
    with open(tmp_path / "mono_out.y4m", "rb") as f:
        r = Y4MReader(f, mono=True)
        assert (r.width, r.height, r.chroma) == (W, H, "400")
        got = np.concatenate(list(r.chunks(16)), 0)
    assert np.array_equal(got.reshape(N, H, W), sr_u8[..., 0])
    with pytest.raises(SystemExit, match="give --chroma-filter bicubic"):
        upscale.main(["-i", str(tmp_path / "in.y4m"), "-o", str(tmp_path / "x.y4m")] + common)
