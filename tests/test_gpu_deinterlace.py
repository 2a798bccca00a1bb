"""GPU checks of the deinterlacer: savsr_video_deinterlace_u8 / _u16 against the numpy specification bit for bit (the shared inputs of
tests/deinterlace_cases.py, the kernels' tile edges, unaligned pointers, ranges with context, planes in place), the entries' refusals,
the property of upscale_video(fields=...) (bit for bit the call on the deinterlaced video), VideoUpscaler(fields=...) under any
chunking, the CLI."""
import io
import os
import re

import numpy as np
import pytest
import torch

import savsr_amd
from savsr_amd import active, y4m, yuv
from savsr_amd.deinterlace import FIELD_ORDERS, deinterlace_frames, deinterlace_matrix
from savsr_amd.utils import synth
from tests.deinterlace_cases import STEPS, input_set, noise, shapes_for
from tests.video_cases import WEIGHT_SEED

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POISON = 0xA5


def _lib():
    from savsr_amd import _lib as L
    return L.load()


def _tile():
    """The kernels' constants: (interpolated rows, bytes of a row) of a vector tile, (interpolated rows, samples of a row) of a
    one-sample tile."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "savsr_amd", "csrc", "deinterlace.hip")).read()
    return tuple(int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) for name in ("DI_TILE_IROWS", "DI_TILE_BYTES", "DI_ONE_IROWS", "DI_ONE_COLS"))


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


def _run(mats, order, step=1, depth=8, rng=None, off=0, before=0, after=0):
    """One entry of the C ABI on the matrices [N, R, C] as the plane `before` bytes into frames of before + plane + after bytes, the
    first frame `off` bytes past a 256-byte aligned allocation; source frames [rng) (default: all).  The output frames have the same
    layout, are poisoned first and are followed by guard bytes: nothing outside the planes is written.  Returns [2 n, R, C]."""
    mats = np.ascontiguousarray(mats)
    n, r, c = mats.shape
    lo, hi = rng or (0, n)
    plane = mats.astype("<u2").view(np.uint8).reshape(n, -1) if depth > 8 else mats.astype(np.uint8).reshape(n, -1)
    fb = before + plane.shape[1] + after
    host = np.full((n, fb), 0x3C, np.uint8)
    host[:, before:before + plane.shape[1]] = plane
    src = torch.empty(n * fb + off + 64, dtype=torch.uint8, device=DEV)
    assert src.data_ptr() % 256 == 0
    src[off:off + n * fb].copy_(torch.from_numpy(host).reshape(-1))
    no = 2 * (hi - lo)
    dst = torch.full((no * fb + off + 64,), POISON, dtype=torch.uint8, device=DEV)
    lib, st = _lib(), torch.cuda.current_stream().cuda_stream
    if depth > 8:
        rc = lib.savsr_video_deinterlace_u16(src.data_ptr() + off, n, fb, before, r, c, depth, FIELD_ORDERS.index(order), lo, hi, dst.data_ptr() + off, fb, before, st)
    else:
        rc = lib.savsr_video_deinterlace_u8(src.data_ptr() + off, n, fb, before, r, c, step, FIELD_ORDERS.index(order), lo, hi, dst.data_ptr() + off, fb, before, st)
    assert rc == 0, lib.savsr_last_error()
    got = dst.cpu().numpy()
    assert (got[:off] == POISON).all() and (got[off + no * fb:] == POISON).all()
    got = got[off:off + no * fb].reshape(no, fb)
    assert (got[:, :before] == POISON).all() and (got[:, before + plane.shape[1]:] == POISON).all()
    got = got[:, before:before + plane.shape[1]]
    return np.ascontiguousarray(got).view("<u2").reshape(no, r, c) if depth > 8 else got.reshape(no, r, c)


def _check(mats, order, step=1, depth=8, **kw):
    want = deinterlace_matrix(mats, order, step, depth)[0]
    lo, hi = kw.get("rng") or (0, mats.shape[0])
    got = _run(mats, order, step, depth, **kw)
    assert np.array_equal(got, want[2 * lo:2 * hi]), (mats.shape, order, step, depth, kw, np.argwhere(got != want[2 * lo:2 * hi])[:4])


# ---------------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_deinterlace_u8_equals_the_spec(order, step):
    """The shared inputs on the spec's shapes.  No row of them is a multiple of 16 bytes, so they take the one-sample form; the vector
    form runs the same inputs in test_deinterlace_u8_vector_form_of_every_step."""
    for r, c in shapes_for(step):
        for name, v in input_set(r, c, step):
            _check(v.astype(np.uint8), order, step)


@pytest.mark.parametrize("depth", [10, 12])
@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_deinterlace_u16_equals_the_spec(order, depth):
    top = (1 << depth) - 1
    for r, c in shapes_for(1):
        for name, v in input_set(r, c, 1, top):
            v = v.astype(np.uint16)
            v[:, ::2, ::5] = 60000                                                   # above 2^d - 1: read as 2^d - 1, copied as they are
            _check(v, order, 1, depth)


def _edge_shapes():
    vr, vb, orows, ocols = _tile()
    assert (vr, vb, orows, ocols) == (16, 256, 4, 64)
    return ([(2 * vr + dr, vb + 16 * dr) for dr in (-1, 0, 1)] +            # the vector tile: 31 x 240, 32 x 256, 33 x 272
            [(2 * orows + dr, ocols + dr) for dr in (-1, 0, 1)] +            # the one-sample tile: 7 x 63, 8 x 64, 9 x 65
            [(2 * vr + 1, 15), (2 * vr, 16), (2 * vr - 1, 17), (9, 48)])      # the 16-byte width: below, at, above; three chunks of step 3


@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_deinterlace_across_the_tile_edges_and_off_alignment(order):
    """Rows and row bytes one below, at and one above the tiles of both forms and the 16-byte width.  A row of a multiple of 16 bytes
    from an aligned pointer takes the vector form; the same matrix one byte (two for 16-bit samples) off takes the one-sample form."""
    for r, c in _edge_shapes():
        v = noise(r, c, 255, seed=r * c)
        v[1, r // 2] = 255
        v[2, :, c // 2] = 0
        for off in (0, 1):
            _check(v.astype(np.uint8), order, 1, off=off)
        if c % 3 == 0:
            _check(v.astype(np.uint8), order, 3)
        if c % 2 == 0:                                                               # the same bytes as 16-bit samples: c / 2 columns
            w = noise(r, c // 2, 1023, seed=r + c).astype(np.uint16)
            w[:, 1::2, ::3] = 4096
            for off in (0, 2):
                _check(w, order, 1, 10, off=off)


@pytest.mark.parametrize("step", [1, 2, 3, 4])
def test_deinterlace_u8_vector_form_of_every_step(step):
    """Rows of 48 pixels x step bytes: a multiple of 16 bytes for every step, three to twelve chunks, so the +-3 step neighbours come from
    the chunks beside a lane's own; the shared inputs, so every branch is taken here too."""
    for name, v in input_set(9, 48 * step, step):
        _check(v.astype(np.uint8), "tff", step)
    _check(input_set(9, 48 * step, step)[2][1].astype(np.uint8), "bff", step)


@pytest.mark.parametrize("depth", [10, 12])
def test_deinterlace_u16_vector_form(depth):
    """Rows of 48 samples, 96 bytes: six chunks of the vector form; the shared inputs, which take every branch at this shape too
    (tests/test_deinterlace.py), with samples above 2^d - 1 among them."""
    top = (1 << depth) - 1
    for name, v in input_set(9, 48, 1, top):
        v = v.astype(np.uint16)
        v[:, ::2, ::5] = 60000
        for order in FIELD_ORDERS:
            _check(v, order, 1, depth)


def test_deinterlace_frame_counts_and_ranges():
    """n_frames 1, 2 and 3, and the range [1, 2) of 3 with its context: prev and next are the resident frames 0 and 2."""
    v = noise(9, 48, 255, seed=8).astype(np.uint8)
    for n in (1, 2, 3):
        for off in (0, 1):
            _check(v[:n], "tff", off=off)
    for rng in ((1, 2), (0, 1), (2, 3), (1, 3)):
        for off in (0, 1):
            _check(v, "bff", rng=rng, off=off)
        _check(noise(9, 24, 4095, seed=9).astype(np.uint16), "tff", 1, 12, rng=rng)
    # the range without its context is another video: frame 1 alone is not frame 1 of three
    assert not np.array_equal(_run(v[1:2], "tff"), deinterlace_matrix(v, "tff")[0][2:4])


@pytest.mark.parametrize("depth", [8, 10])
def test_deinterlace_the_planes_of_i420_frames_in_place(depth):
    """Three calls through the plane offsets and the frame strides; 16 x 32: the Y plane and, at 8 bits, the chroma planes of 8 x 16 are
    16-byte aligned; 7 x 10: none is."""
    for h, w in ((16, 32), (7, 10)):
        fb = yuv.frame_bytes(h, w, depth)
        rng = np.random.RandomState(h + depth)
        if depth == 8:
            frames = rng.randint(0, 256, size=(3, fb), dtype=np.uint8)
        else:
            frames = rng.randint(0, 1 << depth, size=(3, fb // 2)).astype("<u2").view(np.uint8).reshape(3, fb)
        want = deinterlace_frames(frames, "tff", "i420", (h, w), depth)
        got = savsr_amd.deinterlace(torch.from_numpy(frames), "tff", "i420", (h, w), depth)
        assert got.device.type == "cuda" and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
        # one plane at a time through _run: the other planes' bytes of the output stay poisoned
        ch, cw = yuv.chroma_hw(h, w)
        s = 1 if depth == 8 else 2
        planes = yuv.split_planes(frames, h, w, depth)
        before = 0
        for p in planes:
            size = p.shape[1] * p.shape[2] * s
            _check(p, "tff", 1, depth, before=before, after=fb - before - size)
            before += size


def test_public_deinterlace_of_every_frame_kind():
    rng = np.random.RandomState(10)
    rgb = rng.randint(0, 256, size=(3, 9, 16, 3), dtype=np.uint8)
    for order in FIELD_ORDERS:
        assert np.array_equal(savsr_amd.deinterlace(torch.from_numpy(rgb), order).cpu().numpy(), deinterlace_frames(rgb, order))
    on_dev = torch.from_numpy(rgb).to(DEV)
    assert np.array_equal(savsr_amd.deinterlace(on_dev, "bff").cpu().numpy(), deinterlace_frames(rgb, "bff"))
    grey = rng.randint(0, 256, size=(2, 8, 16, 1), dtype=np.uint8)
    assert np.array_equal(savsr_amd.deinterlace(torch.from_numpy(grey), "tff").cpu().numpy(), deinterlace_frames(grey, "tff"))
    for fmt, layout, depth in (("i422", "422", 8), ("i444", "444", 12), ("y400", "400", 10), ("i420", "420", 12)):
        h, w = 9, 14
        fb = yuv.frame_bytes(h, w, depth, layout)
        frames = (rng.randint(0, 256, size=(3, fb), dtype=np.uint8) if depth == 8
                  else rng.randint(0, 1 << depth, size=(3, fb // 2)).astype("<u2").view(np.uint8).reshape(3, fb))
        got = savsr_amd.deinterlace(torch.from_numpy(frames), "tff", fmt, (h, w), depth)
        assert np.array_equal(got.cpu().numpy(), deinterlace_frames(frames, "tff", fmt, (h, w), depth)), fmt


def test_deinterlace_entries_refuse_bad_arguments():
    lib = _lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    out = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p, o = buf.data_ptr(), out.data_ptr()
    u8, u16 = lib.savsr_video_deinterlace_u8, lib.savsr_video_deinterlace_u16
    # (frames, n_frames, frame_bytes, plane_offset, rows, row_bytes | cols, step | depth, order, from, to, out, out_frame_bytes, out_plane_offset)
    bad = [
        (u8, (0, 2, 64, 0, 8, 8, 1, 0, 0, 2, o, 64, 0), "null pointer"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 2, 0, 64, 0), "null pointer"),
        (u8, (p, 0, 64, 0, 8, 8, 1, 0, 0, 0, o, 64, 0), "n_frames >= 1"),
        (u8, (p, 2, 64, 0, 1, 8, 1, 0, 0, 2, o, 64, 0), "rows >= 2"),
        (u8, (p, 2, 64, 0, 8, 0, 1, 0, 0, 2, o, 64, 0), "at least one sample"),
        (u8, (p, 2, 64, 0, 8, 8, 0, 0, 0, 2, o, 64, 0), "step 1 .. 4"),
        (u8, (p, 2, 64, 0, 8, 8, 5, 0, 0, 2, o, 64, 0), "step 1 .. 4"),
        (u8, (p, 2, 64, 0, 8, 8, 3, 0, 0, 2, o, 64, 0), "divisor of row_bytes"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 2, 0, 2, o, 64, 0), "order 0 (tff) or 1 (bff)"),
        (u8, (p, 2, 64, 0, 8, 8, 1, -1, 0, 2, o, 64, 0), "order 0 (tff) or 1 (bff)"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, -1, 2, o, 64, 0), "0 <= from < to <= n_frames"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 3, o, 64, 0), "0 <= from < to <= n_frames"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 1, 1, o, 64, 0), "0 <= from < to <= n_frames"),
        (u8, (p, 2, 63, 0, 8, 8, 1, 0, 0, 2, o, 64, 0), "frame_bytes smaller"),
        (u8, (p, 2, 64, 1, 8, 8, 1, 0, 0, 2, o, 64, 0), "frame_bytes smaller"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 2, o, 63, 0), "out_frame_bytes smaller"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 2, o, 64, 1), "out_frame_bytes smaller"),
        (u8, (p, 2, 64, -1, 8, 8, 1, 0, 0, 2, o, 64, 0), "plane offsets >= 0"),
        (u16, (p, 2, 128, 0, 8, 8, 8, 0, 0, 2, o, 128, 0), "depth 10 or 12"),
        (u16, (p, 2, 128, 0, 8, 8, 14, 0, 0, 2, o, 128, 0), "depth 10 or 12"),
        (u16, (p + 1, 2, 128, 0, 8, 8, 10, 0, 0, 2, o, 128, 0), "2-byte aligned"),
        (u16, (p, 2, 128, 0, 8, 8, 10, 0, 0, 2, o + 1, 128, 0), "2-byte aligned"),
        (u16, (p, 2, 129, 0, 8, 8, 10, 0, 0, 2, o, 128, 0), "2-byte aligned"),
        (u16, (p, 2, 130, 1, 8, 8, 10, 0, 0, 2, o, 128, 0), "2-byte aligned"),
        (u16, (p, 2, 127, 0, 8, 8, 10, 0, 0, 2, o, 128, 0), "frame_bytes smaller"),
        (u16, (p, 2, 128, 0, 1, 8, 10, 0, 0, 2, o, 128, 0), "rows >= 2"),
        (u16, (0, 2, 128, 0, 8, 8, 10, 0, 0, 2, o, 128, 0), "null pointer"),
    ]
    for fn, args, words in bad:
        assert fn(*args, None) == -1, (fn.__name__, args)
        msg = lib.savsr_last_error().decode()
        assert words in msg and fn.__name__[len("savsr_"):] in msg, (fn.__name__, args, msg)
    torch.cuda.synchronize()
    assert not out.any()                                                             # refused before the device is touched


# ---------------------------------------------------------------------------------------------------------------------- the property
H, W, N = 16, 20, 4          # 4 interlaced frames: the 8 progressive ones a 7-frame reflection window needs


def _rgb(seed=5, n=N):
    return np.random.RandomState(seed).randint(0, 256, size=(n, H, W, 3), dtype=np.uint8)


def _planar(layout, depth, seed=6, n=N):
    fb = yuv.frame_bytes(H, W, depth, layout)
    if depth == 8:
        return np.random.RandomState(seed).randint(0, 256, size=(n, fb), dtype=np.uint8)
    return np.random.RandomState(seed).randint(0, 1 << depth, size=(n, fb // 2)).astype("<u2").view(np.uint8).reshape(n, fb)


def _property(net, frames: np.ndarray, kw, more, out, scales=(2,), orders=FIELD_ORDERS):
    """upscale_video(v, fields=o) is upscale_video on the deinterlaced video, the spec's and the GPU's (which are equal)."""
    fmt, size, depth = kw.get("pixel_format", "rgb"), kw.get("size"), kw.get("depth", 8)
    for order in orders:
        prog = deinterlace_frames(frames, order, fmt, size, depth)
        on_gpu = savsr_amd.deinterlace(torch.from_numpy(frames), order, fmt, size, depth)
        assert np.array_equal(on_gpu.cpu().numpy(), prog)
        for scale in scales:
            want = net.upscale_video(torch.from_numpy(prog), scale=scale, out=out, **kw, **more)
            got = net.upscale_video(torch.from_numpy(frames), scale=scale, out=out, fields=order, **kw, **more)
            assert got.shape[0] == 2 * frames.shape[0] and got.shape == want.shape and torch.equal(got, want), (out, order, scale)
            assert torch.equal(net.upscale_video(on_gpu, scale=scale, out=out, **kw, **more), want)


def test_property_uint8(net3):
    _property(net3, _rgb(), {}, {}, "uint8", scales=(2, (2.5, 3.0)))


def test_property_i420(net3):
    _property(net3, _planar("420", 8), dict(pixel_format="i420", size=(H, W)), {}, "i420")


def test_property_i420_10_bits(net3):
    _property(net3, _planar("420", 10), dict(pixel_format="i420", size=(H, W), depth=10), dict(out_depth=10), "i420", orders=("bff",))


def test_property_luma_only_y400(net1):
    _property(net1, _planar(yuv.MONO, 8), dict(pixel_format="y400", size=(H, W)), {}, "y400", orders=("tff",))


def test_property_luma_only_i420_bicubic_chroma(net1):
    """The luma-only path's chroma resampler reads the deinterlaced chroma planes."""
    _property(net1, _planar("420", 8, 7), dict(pixel_format="i420", size=(H, W)), dict(chroma_filter="bicubic"), "i420", orders=("tff",))


def test_fields_none_is_the_call_without_the_argument(net3):
    v = torch.from_numpy(_rgb(8, 8))
    assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", fields=None), net3.upscale_video(v, scale=2, out="uint8"))
    with pytest.raises(ValueError, match="float frames have no integer samples"):
        net3.upscale_video(v.to(DEV).float().permute(0, 3, 1, 2).contiguous() / 255, scale=2, fields="tff")


def test_property_with_cuts(net3):
    """Explicit cuts index the deinterlaced video (a cut at source frame 2 is 4); "auto" scores the progressive frames."""
    v = _rgb(9, 5)
    v[2:] = 255 - v[2:]
    _property(net3, v, {}, dict(cuts=[4]), "uint8", orders=("tff",))
    yy, xx = np.mgrid[0:H, 0:W]                                                      # two still, smooth scenes: the only change is the cut
    a = np.stack([(3 * xx + 5 * yy) % 256, (7 * xx + 2 * yy) % 256, (xx * yy) % 256], -1).astype(np.uint8)
    v = np.stack([a, a, 255 - a, 255 - a, 255 - a])
    prog = torch.from_numpy(deinterlace_frames(v, "tff"))
    assert savsr_amd.detect_cuts(prog) == [4]
    _property(net3, v, {}, dict(cuts="auto"), "uint8", orders=("tff",))
    got = net3.upscale_video(torch.from_numpy(v), scale=2, out="uint8", fields="tff", cuts="auto")
    assert torch.equal(got, net3.upscale_video(prog, scale=2, out="uint8", cuts=[4]))
    with pytest.raises(ValueError, match="cut 10"):                                  # 0 < k < 2 N = 10
        net3.upscale_video(torch.from_numpy(v), scale=2, fields="tff", cuts=[10])


def test_property_with_crop_auto(net3):
    """Deinterlacing comes before the crop: the detector reads the progressive frames."""
    rng = np.random.RandomState(10)
    v = rng.randint(12, 25, size=(N, H, W, 3)).astype(np.uint8)
    v[:, 4:12, 2:18] = rng.randint(60, 256, size=(N, 8, 16, 3))
    prog = deinterlace_frames(v, "tff")
    rows, cols = active.line_sums(prog)                                              # the numpy detector on the spec's progressive frames
    rect = active.active_rect(rows.max(0), cols.max(0), *active.line_samples(H, W, 3))
    # an interpolated row beside a bar's edge is the mean of a bar row and a picture row, which is above the limit: the rect found on the
    # progressive frames is a row taller on either side than the woven picture, and it is the one the call must crop to
    assert rect == (3, 2, 10, 16) and savsr_amd.detect_active_area(torch.from_numpy(prog)) == rect
    assert savsr_amd.detect_active_area(torch.from_numpy(v)) == (4, 2, 8, 16)
    want = net3.upscale_video(torch.from_numpy(prog), scale=2, out="uint8", crop=rect)
    assert torch.equal(net3.upscale_video(torch.from_numpy(v), scale=2, out="uint8", fields="tff", crop="auto"), want)
    _property(net3, v, {}, dict(crop="auto"), "uint8", orders=("tff",))
    _property(net3, v, {}, dict(crop=(4, 2, 8, 16), bars="drop"), "uint8", orders=("bff",))


def test_property_with_the_self_ensemble(net3):
    net3.set_self_ensemble(True)
    try:
        _property(net3, _rgb(11), {}, {}, "uint8", orders=("tff",))
    finally:
        net3.set_self_ensemble(False)


def test_property_in_fp16(net3):
    net3.set_precision("fp16")
    try:
        _property(net3, _planar("420", 8, 12), dict(pixel_format="i420", size=(H, W)), {}, "i420", scales=((2.5, 3.0),), orders=("bff",))
    finally:
        net3.set_precision("fp32")


# ---------------------------------------------------------------------------------------------------------------------- streaming
@pytest.mark.parametrize("chunk", [1, 2, 3])
def test_video_upscaler_with_fields_any_chunking_is_bitwise(net3, chunk):
    from savsr_amd import VideoUpscaler
    n = 7
    u8 = torch.from_numpy(_rgb(13, n))
    whole8 = net3.upscale_video(u8, scale=2, out="uint8", fields="tff")
    up = VideoUpscaler(net3, 2, out="uint8", fields="tff")
    parts = []
    for a in range(0, n, chunk):
        parts.append(up.push(u8[a:a + chunk]))
        held = up._split._src                                                        # the held frame and the one before it, and no more
        assert up._split.held == held.shape[0] <= 2 and held.untyped_storage().nbytes() == held.numel() * held.element_size()
    parts.append(up.finish())
    assert all(p.shape[1:] == whole8.shape[1:] for p in parts)                       # the empty returns have the output's size too
    assert parts[0].shape[0] == (0 if chunk < 3 else 1)          # 1, 2 source frames: 0, 2 progressive ones are final, too few for a window
    assert torch.equal(torch.cat(parts, 0), whole8) and up._buf is None and up._split.held == 0
    yv = torch.from_numpy(_planar("420", 10, 14, n))
    kw = dict(out="i420", pixel_format="i420", size=(H, W), depth=10, out_depth=10)
    whole = net3.upscale_video(yv, scale=2, fields="bff", cuts="auto", crop=(2, 4, 11, 13), **kw)
    up = VideoUpscaler(net3, 2, fields="bff", cuts="auto", crop=(2, 4, 11, 13), **kw)
    parts = [up.push(yv[a:a + chunk]) for a in range(0, n, chunk)] + [up.finish()]
    assert torch.equal(torch.cat(parts, 0), whole), chunk


def test_video_upscaler_of_one_interlaced_frame_with_cuts(net3):
    """One source frame is two progressive ones: too few for a window without cuts, one short scene with them."""
    from savsr_amd import VideoUpscaler
    u8 = torch.from_numpy(_rgb(15, 1))
    up = VideoUpscaler(net3, 2, out="uint8", fields="tff", cuts=[])
    first = up.push(u8)
    assert first.shape == (0, 2 * H, 2 * W, 3)
    assert torch.equal(torch.cat([first, up.finish()], 0), net3.upscale_video(u8, scale=2, out="uint8", fields="tff", cuts=[]))
    up = VideoUpscaler(net3, 2, out="uint8", fields="tff")
    up.push(u8)
    with pytest.raises(ValueError, match="too few"):
        up.finish()


# ---------------------------------------------------------------------------------------------------------------------- the CLI
def test_cli_y4m_fields(net3, tmp_path, capsys):
    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    frames = _planar("420", 8, 16, 5)
    f = io.BytesIO()
    y4m.Y4MWriter(f, W, H, (25, 1), "t", (1, 1)).write(frames)
    src, ckpt = tmp_path / "lr.y4m", tmp_path / "net.pth"
    src.write_bytes(f.getvalue())
    sio.save_network(net3, str(ckpt))
    kw = dict(out="i420", pixel_format="i420", size=(H, W))
    base = ["-i", str(src), "--scale", "2", "--checkpoint", str(ckpt), "--chunk", "2"]

    def expect(sr, fps, tag):
        g = io.BytesIO()
        y4m.Y4MWriter(g, 2 * W, 2 * H, fps, tag, y4m.scaled_aspect((1, 1), (H, W), (2 * H, 2 * W))).write(sr.cpu().numpy())
        return g.getvalue()

    # --fields auto: It -> tff, the output is progressive at twice the rate and holds 2 N frames
    dst = tmp_path / "sr50p.y4m"
    assert main(base + ["-o", str(dst), "--fields", "auto"]) == 0
    want = expect(net3.upscale_video(torch.from_numpy(frames), scale=2, fields="tff", **kw), (50, 1), "p")
    assert dst.read_bytes() == want and b" F50:1 Ip " in want[:80]
    assert "treated as progressive" not in capsys.readouterr().err
    # an explicit order overrides the tag
    dst = tmp_path / "sr_bff.y4m"
    assert main(base + ["-o", str(dst), "--fields", "bff"]) == 0
    assert dst.read_bytes() == expect(net3.upscale_video(torch.from_numpy(frames[:]), scale=2, fields="bff", **kw), (50, 1), "p")
    # without the flag: the woven frames as ever, the tag passed through, one line on stderr
    capsys.readouterr()
    dst = tmp_path / "sr_woven.y4m"
    frames8 = _planar("420", 8, 17, 8)
    f = io.BytesIO()
    y4m.Y4MWriter(f, W, H, (25, 1), "t", (1, 1)).write(frames8)
    src.write_bytes(f.getvalue())
    assert main(base + ["-o", str(dst)]) == 0
    err = capsys.readouterr().err
    assert err.count("treated as progressive") == 1 and "--fields" in err
    want = expect(net3.upscale_video(torch.from_numpy(frames8), scale=2, **kw), (25, 1), "t")
    assert dst.read_bytes() == want and b" F25:1 It " in want[:80]
    dst2 = tmp_path / "sr_prog.y4m"
    assert main(base + ["-o", str(dst2), "--fields", "progressive"]) == 0
    assert dst2.read_bytes() == want and "treated as progressive" not in capsys.readouterr().err
    # a PNG-folder output of an interlaced input holds 2 N files
    out_dir = tmp_path / "png"
    assert main(base + ["-o", str(out_dir), "--fields", "tff"]) == 0
    assert sorted(os.listdir(out_dir)) == [f"{k:08d}.png" for k in range(16)]
    # Im (mixed) is refused by name
    f = io.BytesIO()
    y4m.Y4MWriter(f, W, H, (25, 1), "m", (1, 1)).write(frames8)
    src.write_bytes(f.getvalue())
    with pytest.raises(SystemExit, match="Im"):
        main(base + ["-o", str(tmp_path / "x.y4m"), "--fields", "auto"])
