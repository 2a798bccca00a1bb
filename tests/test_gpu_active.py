"""GPU checks of the active-picture path: the three savsr_video_line_sums_* entries against the numpy specification (exact integers),
the detector on constructed letterbox / pillarbox / window-box videos, the crop property of upscale_video(crop=...) (bit for bit the call
on the hand-cropped video; bars="keep" = active.insert_frames of it), VideoUpscaler(crop=...) under any chunking, the CLI."""
import io
import os
import re

import numpy as np
import pytest
import torch

import savsr_amd
from savsr_amd import active, y4m, yuv
from savsr_amd.packing import get_hw
from savsr_amd.utils import synth
from tests.video_cases import WEIGHT_SEED

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POISON = 0x5A5A5A5A


def _lib():
    from savsr_amd import _lib as L
    return L.load()


def _tile():
    """(rows, bytes of a row in the vector form, samples of a row in the one-sample form) of a workgroup's tile: the kernel's constants."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "savsr_amd", "csrc", "active.hip")).read()
    return tuple(int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) for name in ("LS_TILE_ROWS", "LS_TILE_BYTES", "LS_ONE_COLS"))


def _net(**cfg):
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR(**cfg)
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=WEIGHT_SEED), strict=True)
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def net3():
    return _net()


@pytest.fixture(scope="module")
def net1():
    return _net(num_in_ch=1, num_feat=32)


def _offset_copy(host: np.ndarray, off_bytes: int) -> torch.Tensor:
    """The array's bytes on the device, `off_bytes` past the start of an allocation (allocations are at least 256-byte aligned)."""
    flat = torch.from_numpy(np.ascontiguousarray(host)).reshape(-1).view(torch.uint8)
    buf = torch.empty(flat.numel() + off_bytes + 64, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    view = buf[off_bytes:off_bytes + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() == buf.data_ptr() + off_bytes
    return view


def _raw(entry, ptr, n, rows, cols, *args):
    """One entry of the C ABI on a device pointer; both outputs are poisoned first (the entry zeroes them itself) and have a guard cell
    behind them (nothing beyond n * rows / n * cols cells is written)."""
    lib = _lib()
    rs = torch.full((n * rows + 1,), POISON, dtype=torch.int32, device=DEV)
    cs = torch.full((n * cols + 1,), POISON, dtype=torch.int32, device=DEV)
    rc = getattr(lib, entry)(ptr, n, *args, rs.data_ptr(), cs.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.savsr_last_error()
    rs, cs = rs.cpu().numpy().view(np.uint32).astype(np.int64), cs.cpu().numpy().view(np.uint32).astype(np.int64)
    assert rs[-1] == POISON and cs[-1] == POISON
    return rs[:-1].reshape(n, rows), cs[:-1].reshape(n, cols)


def _check_u8(v: np.ndarray, off: int = 0):
    """[N, h, w, c] uint8 frames through savsr_video_line_sums_u8 as h x (w * c) byte matrices, and through savsr_amd.line_sums."""
    n, h, w, c = v.shape
    want_r, want_c = active.line_sums(v)
    want_bytes = v.astype(np.int64).sum(1).reshape(n, w * c)          # per byte column, before the channels are folded
    dv = _offset_copy(v, off)
    rows, cols = _raw("savsr_video_line_sums_u8", dv.data_ptr(), n, h, w * c, h * w * c, h, w * c)
    assert np.array_equal(rows, want_r), (v.shape, off)
    assert np.array_equal(cols, want_bytes), (v.shape, off)
    got = savsr_amd.line_sums(dv.view(n, h, w, c))
    assert all(t.dtype == torch.int64 and t.device == dv.device for t in got)
    assert np.array_equal(got[0].cpu().numpy(), want_r) and np.array_equal(got[1].cpu().numpy(), want_c), (v.shape, off)


# ---------------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("h,w,c", [(5, 3, 3), (181, 319, 1), (64, 48, 1), (16, 32, 3)])
def test_line_sums_u8_equals_the_spec(h, w, c):
    """N = 3 so that frames cannot leak into each other; full-range samples.  5 x 3 x 3 and 181 x 319 take the one-sample form (a row's
    bytes are no multiple of 16), 64 x 48 and 16 x 32 x 3 the vector form; every buffer again one byte off (the one-sample form)."""
    v = np.random.RandomState(h * 7 + w + c).randint(0, 256, size=(3, h, w, c), dtype=np.uint8)
    v[1, h // 2] = 255
    v[2, :, w // 2] = 0
    _check_u8(v)
    _check_u8(v, off=1)
    assert np.array_equal(savsr_amd.line_sums(torch.from_numpy(v))[0].cpu().numpy(), active.line_sums(v)[0])          # host frames


@pytest.mark.parametrize("form", ["vector", "one", "vector+16"])
def test_line_sums_u8_across_the_tile_edges(form):
    """3 rows taller and 5 byte columns wider than a workgroup's tile, of the vector form and of the one-sample form: two tiles along
    both axes, so both atomics paths (rows and columns) add the partials of several workgroups and the tile edges are crossed.  A row
    of tile + 5 bytes is no multiple of 16, so those two shapes run the one-sample kernel; "vector+16" is the nearest wider shape the
    vector kernel itself takes (and, one byte off, the other kernel on the same sizes)."""
    rows, vec_bytes, one_cols = _tile()
    assert rows >= 64
    width = {"vector": vec_bytes + 5, "one": one_cols + 5, "vector+16": vec_bytes + 16}[form]
    v = np.random.RandomState(len(form)).randint(0, 256, size=(3, rows + 3, width, 1), dtype=np.uint8)
    v[0] = 255                                                                    # the largest sums a tile can hold
    _check_u8(v)
    _check_u8(v, off=1)


@pytest.mark.parametrize("h,w,depth", [(12, 16, 10), (33, 50, 12)])
def test_line_sums_u16_equals_the_spec(h, w, depth):
    rng = np.random.RandomState(h + w)
    fb = yuv.frame_bytes(h, w, depth)
    s = rng.randint(0, 1 << depth, size=(3, fb // 2)).astype(np.uint16)
    s[:, ::7] = rng.randint(1 << depth, 1 << 16, size=s[:, ::7].shape)           # above 2^d - 1 (1023 at 10 bits): read as 2^d - 1
    frames = s.astype("<u2").view(np.uint8).reshape(3, fb)
    want = active.line_sums(frames, "i420", (h, w), depth)
    for off in (0, 2):                                                            # 12 x 16 aligned: the vector form; two bytes off: the other
        dv = _offset_copy(frames, off)
        rows, cols = _raw("savsr_video_line_sums_u16", dv.data_ptr(), 3, h, w, fb, h, w, depth)
        assert np.array_equal(rows, want[0]) and np.array_equal(cols, want[1]), (h, w, depth, off)
    got = savsr_amd.line_sums(torch.from_numpy(frames), "i420", (h, w), depth)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])


@pytest.mark.parametrize("n,c,h,w", [(3, 3, 7, 9), (2, 3, 16, 32)])
def test_line_sums_f32_equals_the_spec(n, c, h, w):
    rng = np.random.RandomState(h * w)
    v = rng.uniform(-0.5, 1.5, size=(n, c, h, w)).astype(np.float32)
    v.reshape(-1)[::11] = (rng.randint(0, 255, size=v.reshape(-1)[::11].shape).astype(np.float32) + np.float32(0.5)) / np.float32(255)      # ties
    v[0, 0, 0, 0], v[0, 1, 2, 3], v[0, 2, 4, 5] = np.nan, -0.5, 1.5
    want = active.line_sums(v)
    q = active.line_sums(v.reshape(n * c, 1, h, w))                               # per plane, before the channels are summed
    for off in (0, 4):                                                            # one float off a 16-byte boundary: the one-sample form
        dv = _offset_copy(v, off)
        rows, cols = _raw("savsr_video_line_sums_f32", dv.data_ptr(), n * c, h, w, h, w)
        assert np.array_equal(rows, q[0]) and np.array_equal(cols, q[1]), (n, c, h, w, off)
    got = savsr_amd.line_sums(torch.from_numpy(v).to(DEV))
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])


def test_line_sums_entries_refuse_bad_arguments():
    lib = _lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    out = torch.zeros(256, dtype=torch.int32, device=DEV)
    p, r, c = buf.data_ptr(), out.data_ptr(), out.data_ptr() + 512
    E_ARG, E_ALIGN = -1, -2
    bad = [
        (lib.savsr_video_line_sums_u8, (0, 1, 64, 8, 8, r, c, None), E_ARG, "null pointer"),
        (lib.savsr_video_line_sums_u8, (p, 1, 64, 8, 8, 0, c, None), E_ARG, "null pointer"),
        (lib.savsr_video_line_sums_u8, (p, 1, 64, 8, 8, r, 0, None), E_ARG, "null pointer"),
        (lib.savsr_video_line_sums_u8, (p, 0, 64, 8, 8, r, c, None), E_ARG, "n, rows, row_bytes >= 1"),
        (lib.savsr_video_line_sums_u8, (p, 1, 64, 0, 8, r, c, None), E_ARG, "n, rows, row_bytes >= 1"),
        (lib.savsr_video_line_sums_u8, (p, 1, 63, 8, 8, r, c, None), E_ARG, "frame_bytes smaller"),
        (lib.savsr_video_line_sums_u16, (p, 1, 128, 8, 8, 8, r, c, None), E_ARG, "depth 10 or 12"),
        (lib.savsr_video_line_sums_u16, (p, 1, 128, 8, 8, 14, r, c, None), E_ARG, "depth 10 or 12"),
        (lib.savsr_video_line_sums_u16, (p + 1, 1, 128, 8, 8, 10, r, c, None), E_ALIGN, "2-byte aligned"),
        (lib.savsr_video_line_sums_u16, (p, 0, 128, 8, 8, 10, r, c, None), E_ARG, "n, rows, cols >= 1"),
        (lib.savsr_video_line_sums_u16, (p, 1, 128, 0, 8, 10, r, c, None), E_ARG, "n, rows, cols >= 1"),
        (lib.savsr_video_line_sums_u16, (0, 1, 128, 8, 8, 10, r, c, None), E_ARG, "null pointer"),
        (lib.savsr_video_line_sums_f32, (0, 1, 8, 8, r, c, None), E_ARG, "null pointer"),
        (lib.savsr_video_line_sums_f32, (p, 0, 8, 8, r, c, None), E_ARG, "n_mats, rows, cols >= 1"),
        (lib.savsr_video_line_sums_f32, (p, 1, 0, 8, r, c, None), E_ARG, "n_mats, rows, cols >= 1"),
    ]
    for fn, args, code, words in bad:
        assert fn(*args) == code, (fn.__name__, args)
        assert words in lib.savsr_last_error().decode(), (fn.__name__, args, lib.savsr_last_error())
    assert not out.any()                                                          # refused before the device is touched


# ---------------------------------------------------------------------------------------------------------------------- the detector
def _boxed(rect, n=9, h=24, w=32, seed=0):
    """[n, h, w, 3] uint8 samples: bars of value 16 plus noise in 12 .. 24 (every bar line's mean is at most 24), picture samples in
    60 .. 255."""
    rng = np.random.RandomState(seed)
    y0, x0, ah, aw = rect
    v = rng.randint(12, 25, size=(n, h, w, 3)).astype(np.uint8)
    v[:, y0:y0 + ah, x0:x0 + aw] = rng.randint(60, 256, size=(n, ah, aw, 3))
    return v


LETTERBOX, PILLARBOX, WINDOWBOX = (4, 0, 16, 32), (0, 6, 24, 20), (4, 6, 16, 20)


def _all_kinds(v):
    """The samples as uint8 RGB frames, as the Y plane of I420 frames at 8 and at 10 bits (channel 0; the two low bits and the chroma
    planes random) and as float frames (v / 255 quantises back to v): (frames, line_sums arguments, the samples the detector reads)."""
    n, h, w, _ = v.shape
    rng = np.random.RandomState(1)
    y = v[..., 0]
    c8 = rng.randint(0, 256, size=(n, yuv.frame_bytes(h, w) - h * w), dtype=np.uint8)
    i8 = np.concatenate([y.reshape(n, -1), c8], 1)
    y10 = (y.astype(np.uint16) << 2) | rng.randint(0, 4, size=y.shape).astype(np.uint16)
    c10 = rng.randint(0, 1024, size=c8.shape).astype(np.uint16)
    i10 = np.concatenate([y10.reshape(n, -1), c10], 1).astype("<u2").view(np.uint8).reshape(n, -1)
    unit = np.ascontiguousarray((v.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2))
    yuv_kw = dict(pixel_format="i420", size=(h, w))
    return [(torch.from_numpy(v), {}, v), (torch.from_numpy(i8), yuv_kw, y[..., None]), (torch.from_numpy(i10), dict(yuv_kw, depth=10), y[..., None]),
            (torch.from_numpy(unit).to(DEV), {}, v)]


@pytest.mark.parametrize("rect", [LETTERBOX, PILLARBOX, WINDOWBOX])
def test_detector_finds_the_constructed_rect(rect):
    v = _boxed(rect)
    for frames, kw, samples in _all_kinds(v):
        rows, cols = active.line_sums(frames, **kw)
        assert np.array_equal(rows, active.line_sums(samples)[0])                 # every kind holds the constructed samples
        s_row, s_col = active.line_samples(24, 32, samples.shape[3])
        outside = np.ones(24, bool)
        outside[rect[0]:rect[0] + rect[2]] = False
        assert (rows.max(0)[outside] <= 24 * s_row).all() and (rows.max(0)[~outside] >= 60 * s_row).all()          # the construction
        assert active.align_rect(active.active_rect(rows.max(0), cols.max(0), s_row, s_col), "420" if kw else None) == rect, kw
        assert savsr_amd.detect_active_area(frames, **kw) == rect, kw             # the GPU finds the constructed rect
    assert savsr_amd.detect_active_area(torch.from_numpy(v), limit=250) == (0, 0, 24, 32)          # nothing above the limit: the whole frame


def test_a_bright_line_in_one_frame_widens_the_rect():
    v = _boxed(LETTERBOX)
    v[5, 1] = 200                                                                 # inside the top bar, in one frame of nine
    for frames, kw, _ in _all_kinds(v):
        got = savsr_amd.detect_active_area(frames, **kw)
        assert got == ((0, 0, 20, 32) if kw else (1, 0, 19, 32)), kw              # 4:2:0: the offset moves outwards to the block


# ---------------------------------------------------------------------------------------------------------------------- the property
H, W, RECT, N = 16, 20, (2, 4, 11, 13), 8
SCALES = (2, (2.5, 3.0))


def _rgb(seed=5):
    return np.random.RandomState(seed).randint(0, 256, size=(N, H, W, 3), dtype=np.uint8)


def _planar(layout, depth, seed=6):
    fb = yuv.frame_bytes(H, W, depth, layout)
    if depth == 8:
        return np.random.RandomState(seed).randint(0, 256, size=(N, fb), dtype=np.uint8)
    s = np.random.RandomState(seed).randint(0, 1 << depth, size=(N, fb // 2)).astype("<u2")
    return s.view(np.uint8).reshape(N, fb)


def _property(net, frames, kw, crop_kw, out, out_depth=8, out_colour="bt601", scales=SCALES, crop=RECT):
    """upscale_video(crop=R, bars="drop") is upscale_video of the hand crop; bars="keep" is active.insert_frames of that."""
    fmt, size, depth = kw.get("pixel_format", "rgb"), kw.get("size"), kw.get("depth", 8)
    for scale in scales:
        sc = (float(scale), float(scale)) if not isinstance(scale, tuple) else scale
        host = frames.cpu().numpy() if isinstance(frames, torch.Tensor) else frames
        cropped = np.ascontiguousarray(active.crop_frames(host, RECT, fmt, size, depth))
        dev = DEV if isinstance(frames, torch.Tensor) and frames.is_cuda else None
        hand = torch.from_numpy(cropped).to(dev) if dev else torch.from_numpy(cropped)
        want = net.upscale_video(hand, scale=scale, out=out, **dict(kw, **({"size": RECT[2:]} if size else {})), **crop_kw)
        drop = net.upscale_video(frames, scale=scale, out=out, crop=crop, bars="drop", **kw, **crop_kw)
        assert drop.shape == want.shape and torch.equal(drop, want), (out, scale, "drop")
        keep = net.upscale_video(frames, scale=scale, out=out, crop=crop, **kw, **crop_kw)
        out_layout = yuv.CHROMA_OF.get(out) or (yuv.MONO if out == "y400" else None)
        full = active.insert_frames(want, active.place(RECT, H, W, sc, out_layout), out, out_depth, out_colour)
        plain = net.upscale_video(frames, scale=scale, out=out, **kw, **crop_kw)
        assert keep.shape == plain.shape == full.shape and np.array_equal(keep.cpu().numpy(), full), (out, scale, "keep")


def test_property_uint8(net3):
    _property(net3, torch.from_numpy(_rgb()), {}, {}, "uint8")


def test_property_float(net3):
    fl = (torch.from_numpy(_rgb()).to(DEV).float() / 255).permute(0, 3, 1, 2).contiguous()
    _property(net3, fl, {}, {}, "float")


def test_property_i420(net3):
    _property(net3, torch.from_numpy(_planar("420", 8)), dict(pixel_format="i420", size=(H, W)), {}, "i420")


def test_property_i420_10_bits_to_i444(net3):
    _property(net3, torch.from_numpy(_planar("420", 10)), dict(pixel_format="i420", size=(H, W), depth=10), dict(out_depth=10), "i444", out_depth=10)


def test_property_i422_left_sited(net3):
    _property(net3, torch.from_numpy(_planar("422", 8)), dict(pixel_format="i422", size=(H, W), siting="left"), dict(out_siting="left"), "i422")


def test_property_luma_only_y400(net1):
    _property(net1, torch.from_numpy(_planar(yuv.MONO, 8)), dict(pixel_format="y400", size=(H, W)), {}, "y400")


def test_property_luma_only_i420_bicubic_chroma(net1):
    _property(net1, torch.from_numpy(_planar("420", 8)), dict(pixel_format="i420", size=(H, W)), dict(chroma_filter="bicubic"), "i420")


def test_property_with_the_self_ensemble(net3):
    net3.set_self_ensemble(True)
    try:
        _property(net3, torch.from_numpy(_rgb(7)), {}, {}, "uint8", scales=(2,))
    finally:
        net3.set_self_ensemble(False)


def test_property_in_fp16(net3):
    net3.set_precision("fp16")
    try:
        _property(net3, torch.from_numpy(_planar("420", 8, 8)), dict(pixel_format="i420", size=(H, W)), {}, "i420", scales=((2.5, 3.0),))
    finally:
        net3.set_precision("fp32")


def test_property_with_auto_cuts(net3):
    """Two still scenes with a cut at frame 4 inside the rect, and bars that flip at frame 2: the crop comes first, so the cut detector
    sees the picture's cut alone."""
    v = _rgb(9)
    v[:4] = v[:1]
    v[4:] = 255 - v[:1]
    y0, x0, ah, aw = RECT
    inside = v[:, y0:y0 + ah, x0:x0 + aw].copy()
    v[:2], v[2:] = 0, 255
    v[:, y0:y0 + ah, x0:x0 + aw] = inside
    assert savsr_amd.detect_cuts(torch.from_numpy(np.ascontiguousarray(inside))) == [4]
    assert savsr_amd.detect_cuts(torch.from_numpy(v)) != [4]
    _property(net3, torch.from_numpy(v), {}, dict(cuts="auto"), "uint8", scales=(2,))
    got = net3.upscale_video(torch.from_numpy(v), scale=2, out="uint8", crop=RECT, bars="drop", cuts="auto")
    assert torch.equal(got, net3.upscale_video(torch.from_numpy(np.ascontiguousarray(inside)), scale=2, out="uint8", cuts=[4]))


def test_crop_auto_on_a_letterboxed_video(net3):
    v = _boxed(LETTERBOX)
    u8 = torch.from_numpy(v)
    assert savsr_amd.detect_active_area(u8) == LETTERBOX
    hand = torch.from_numpy(np.ascontiguousarray(active.crop_frames(v, LETTERBOX)))
    want = net3.upscale_video(hand, scale=2, out="uint8")
    assert torch.equal(net3.upscale_video(u8, scale=2, out="uint8", crop="auto", bars="drop"), want)
    assert torch.equal(net3.upscale_video(u8, scale=2, out="uint8", crop=LETTERBOX, bars="drop"), want)
    keep = net3.upscale_video(u8, scale=2, out="uint8", crop="auto")
    assert np.array_equal(keep.cpu().numpy(), active.insert_frames(want, active.place(LETTERBOX, 24, 32, (2.0, 2.0), None), "uint8"))
    assert keep.shape == (9, 48, 64, 3) and not keep[:, :8].any() and not keep[:, 40:].any()
    # a limit that finds nothing is the whole frame, which is the uncropped call
    assert torch.equal(net3.upscale_video(u8, scale=2, out="uint8", crop="auto", crop_limit=250), net3.upscale_video(u8, scale=2, out="uint8"))
    assert torch.equal(net3.upscale_video(u8, scale=2, out="uint8", crop=(0, 0, 24, 32), bars="drop"), net3.upscale_video(u8, scale=2, out="uint8"))


# ---------------------------------------------------------------------------------------------------------------------- streaming
@pytest.mark.parametrize("bars", ["keep", "drop"])
def test_video_upscaler_with_a_crop_any_chunking_is_bitwise(net3, bars):
    from savsr_amd import VideoUpscaler
    n = 16
    fb = yuv.frame_bytes(H, W)
    yv = torch.from_numpy(np.random.RandomState(11).randint(0, 256, size=(n, fb), dtype=np.uint8))
    kw = dict(out="i420", pixel_format="i420", size=(H, W))
    whole = net3.upscale_video(yv, scale=2, crop=RECT, bars=bars, **kw)
    u8 = torch.from_numpy(np.random.RandomState(12).randint(0, 256, size=(n, H, W, 3), dtype=np.uint8))
    whole8 = net3.upscale_video(u8, scale=(2.5, 3.0), out="uint8", crop=RECT, bars=bars)
    for chunk in (1, 3, 16):
        up = VideoUpscaler(net3, 2, crop=RECT, bars=bars, **kw)
        parts = [up.push(yv[a:a + chunk]) for a in range(0, n, chunk)] + [up.finish()]
        assert all(p.shape[1] == whole.shape[1] for p in parts)                    # the empty returns have the full / the picture's size too
        assert torch.equal(torch.cat(parts, 0), whole), (bars, chunk)
        up = VideoUpscaler(net3, (2.5, 3.0), out="uint8", crop=RECT, bars=bars)
        parts = [up.push(u8[a:a + chunk]) for a in range(0, n, chunk)] + [up.finish()]
        assert all(p.shape[1:] == whole8.shape[1:] for p in parts)
        assert torch.equal(torch.cat(parts, 0), whole8), (bars, chunk)
        assert up._buf is None and up.spec.size is None


# ---------------------------------------------------------------------------------------------------------------------- the CLI
def test_cli_y4m_crop_auto_bars_drop(net3, tmp_path, capsys):
    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    h, w = 24, 32
    frames = _all_kinds(_boxed(LETTERBOX))[1][0].numpy()                          # I420 frames whose Y plane holds the boxed samples
    f = io.BytesIO()
    y4m.Y4MWriter(f, w, h, (30, 1), "p", (1, 1)).write(frames)
    src, dst, ckpt = tmp_path / "lr.y4m", tmp_path / "sr.y4m", tmp_path / "net.pth"
    src.write_bytes(f.getvalue())
    sio.save_network(net3, str(ckpt))
    assert main(["-i", str(src), "-o", str(dst), "--scale", "2", "--checkpoint", str(ckpt), "--chunk", "4", "--crop", "auto", "--bars", "drop"]) == 0
    assert "--crop auto: active picture 16 x 32 at (4, 0): --crop 4,0,16,32" in capsys.readouterr().err
    kw = dict(out="i420", pixel_format="i420", size=(h, w))
    sr = net3.upscale_video(torch.from_numpy(frames), scale=2, crop="auto", bars="drop", **kw).cpu().numpy()
    Ha, Wa = get_hw(16, 32, (2, 2))
    g = io.BytesIO()
    y4m.Y4MWriter(g, Wa, Ha, (30, 1), "p", y4m.scaled_aspect((1, 1), (16, 32), (Ha, Wa))).write(sr)
    assert dst.read_bytes() == g.getvalue() and g.getvalue().startswith(b"YUV4MPEG2 W64 H32 ")
    # bars kept: the full-size frames of the Python call
    dst2 = tmp_path / "sr_keep.y4m"
    assert main(["-i", str(src), "-o", str(dst2), "--scale", "2", "--checkpoint", str(ckpt), "--crop", "4,0,16,32"]) == 0
    keep = net3.upscale_video(torch.from_numpy(frames), scale=2, crop=LETTERBOX, **kw).cpu().numpy()
    g = io.BytesIO()
    y4m.Y4MWriter(g, 64, 48, (30, 1), "p", y4m.scaled_aspect((1, 1), (h, w), (48, 64))).write(keep)
    assert dst2.read_bytes() == g.getvalue()
    with pytest.raises(SystemExit):                                               # stdin allows no first pass
        main(["-i", "-", "-o", str(tmp_path / "x.y4m"), "--scale", "2", "--checkpoint", str(ckpt), "--crop", "auto"])
    assert "--crop auto needs a first pass over the input" in capsys.readouterr().err

