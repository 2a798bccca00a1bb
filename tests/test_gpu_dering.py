"""GPU checks of the deringing stage: savsr_video_dering_u8 / _u16 against the numpy specification bit for bit between guard bytes and
into poisoned output (the shared generators and shapes of tests/dering_cases.py: the smallest planes, one tile plus a row and a column,
two tiles each way with a ragged rest; progressive and field-wise with 1, 2 and 17 rows; steps 1, 3 and 4; 1 and 3 frames; a plane inside
a frame at a misaligned base; every depth with samples above it; the strengths (0, 0), (0, 2), (4, 0), (15, 4) and the defaults on the
case picture, on noise and on constant blocks; dampings 3 and 6), the entries' refusals, `dering_video` on every frame kind, the command
line on a Y4M file, and the properties of upscale_video(dering=...): bit for bit the call on the filtered video, behind deblock= (and not
in front of it), in front of fields=, pulldown=, the crop and both denoisers, field-wise exactly when the video is treated as
interlaced, with scan="detect", and in VideoUpscaler under any chunking."""
import io

import numpy as np
import pytest
import torch

import savsr_amd
from savsr_amd import y4m, yuv
from savsr_amd.dering import dering_frames, dering_plane
from savsr_amd.utils import synth
from tests.dering_cases import (DAMPINGS, DEPTHS, FIELD_ROWS, SMALL, STRENGTHS, TIE_SHAPE, as_bytes, case_frames, constant_blocks, one_tile_plus,
                                two_tiles_ragged)
from tests.scan_cases import packed_case, planar_case
from tests.video_cases import WEIGHT_SEED

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POISON = 0xA5


def _lib():
    from savsr_amd import _lib as L
    return L.load()


@pytest.fixture(scope="module")
def net3():
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=WEIGHT_SEED), strict=True)
    return net.to(DEV).eval()


def _run(m, depth=8, strength=(4, 2), damping=5, interlaced=False, off=0, before=0, after=0):
    """One entry on the samples [N, R, C, step] as the plane `before` bytes into frames of before + plane + after bytes, the first frame
    `off` bytes past a 256-byte aligned allocation.  The output frames have the same layout, are poisoned first and are followed by
    guard bytes: nothing outside the planes is written.  Returns [N, R, C, step]."""
    n, r, c, step = m.shape
    plane = as_bytes(m)
    fb = before + plane.shape[1] + after
    host = np.full((n, fb), 0x3C, np.uint8)
    host[:, before:before + plane.shape[1]] = plane
    src = torch.empty(n * fb + off + 64, dtype=torch.uint8, device=DEV)
    assert src.data_ptr() % 256 == 0
    src[off:off + n * fb].copy_(torch.from_numpy(host).reshape(-1))
    dst = torch.full((n * fb + off + 64,), POISON, dtype=torch.uint8, device=DEV)
    assert dst.data_ptr() % 256 == 0
    lib, st, sh = _lib(), torch.cuda.current_stream().cuda_stream, depth - 8
    head = (src.data_ptr() + off, n, fb, before, r, c, step)
    tail = (int(interlaced), strength[0] << sh, strength[1] << sh, damping, dst.data_ptr() + off, fb, before, st)
    rc = lib.savsr_video_dering_u16(*head, depth, *tail) if depth > 8 else lib.savsr_video_dering_u8(*head, *tail)
    assert rc == 0, lib.savsr_last_error()
    got = dst.cpu().numpy()
    assert (got[:off] == POISON).all() and (got[off + n * fb:] == POISON).all()
    got = got[off:off + n * fb].reshape(n, fb)
    assert (got[:, :before] == POISON).all() and (got[:, before + plane.shape[1]:] == POISON).all()
    got = np.ascontiguousarray(got[:, before:before + plane.shape[1]])
    return got.view("<u2").reshape(m.shape) if depth > 8 else got.reshape(m.shape)


def _want(m, depth, strength, damping, interlaced):
    out = np.empty_like(m)
    for t in range(m.shape[0]):
        for ch in range(m.shape[3]):
            out[t, :, :, ch] = dering_plane(m[t, :, :, ch], depth, strength, damping, interlaced)
    return out


def _check(m, depth=8, strength=(4, 2), damping=5, interlaced=False, **place):
    got, want = _run(m, depth, strength, damping, interlaced, **place), _want(m, depth, strength, damping, interlaced)
    assert np.array_equal(got, want), (m.shape, depth, strength, damping, interlaced, place, np.argwhere(got != want)[:4].tolist())
    return got


# ---------------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("interlaced", [False, True])
def test_entries_equal_the_spec_at_the_small_shapes(interlaced):
    """1 x 1, 1 x 9, 9 x 1, 7 x 7, 8 x 8 and 9 x 9 (partial blocks of clamped copies), field-wise also 1, 2 and 17 rows (fields of 1 and 0,
    1 and 1, 9 and 8 rows), and one tile plus a row and a column, at 8 and at 10 bits."""
    rng = np.random.default_rng(100 + interlaced)
    for r, c in SMALL + tuple((r, 21) for r in FIELD_ROWS) + ((3, 17), (35, 21)):
        _check(case_frames(rng, 1, r, c, kind="noise"), 8, (4, 2), 5, interlaced)
        _check(case_frames(rng, 1, r, c), 8, (15, 4), 5, interlaced)
    m = case_frames(rng, 1, *one_tile_plus(1))
    assert not np.array_equal(_check(m, 8, (4, 2), 5, interlaced), m)
    _check(case_frames(rng, 1, 37, 41, depth=10, above=True), 10, (4, 2), 5, interlaced)


@pytest.mark.parametrize("interlaced", [False, True])
def test_two_tiles_each_way_with_a_ragged_rest(interlaced):
    rng = np.random.default_rng(20 + interlaced)
    r, c = two_tiles_ragged(1)
    m = case_frames(rng, 1, r, c)
    assert not np.array_equal(_check(m, 8, (4, 2), 5, interlaced), m)


@pytest.mark.parametrize("depth", DEPTHS)
def test_every_depth_strength_and_damping(depth):
    """(0, 0): min(s, 2^d - 1) comes back; the secondary taps alone, the primary ones alone, the largest strengths and the defaults, on
    the case picture (every branch of the strengths), on uniform noise (the constraint cuts nearly every tap) and on constant blocks (the
    tie rule); dampings 3 and 6.  16-bit planes carry samples above 2^d - 1, which are read as 2^d - 1."""
    rng = np.random.default_rng(30 + depth)
    top = (1 << depth) - 1
    for strength in STRENGTHS:
        for kind in ("case", "noise", "blocks"):
            m = case_frames(rng, 1, 35, 45, depth=depth, above=True, kind=kind)
            for interlaced in (False, True):
                got = _check(m, depth, strength, 5, interlaced)
                if strength == (0, 0):
                    assert np.array_equal(got, np.minimum(m, top))
    for damping in DAMPINGS:
        m = case_frames(rng, 1, 35, 45, depth=depth, above=True)
        a = _check(m, depth, (15, 4), damping)
        _check(case_frames(rng, 1, 19, 23, depth=depth, kind="noise"), depth, (7, 1), damping, True)
    assert not np.array_equal(a, _run(m, depth, (15, 4), 3))          # (a is damping 6's result)
    if depth > 8:
        assert (_run(np.full((1, 19, 20, 1), 0xFFFF, np.uint16), depth) == top).all()


def test_the_tie_rule_on_constant_blocks():
    """Every block has eight equal costs: direction 0, and the secondary taps along directions 2 and 6 smooth across the block borders."""
    m = constant_blocks(*TIE_SHAPE)[None, :, :, None]
    got = _check(m)
    assert 0 < np.count_nonzero(got != m) < m.size // 4


def test_steps_frames_and_a_misaligned_plane_inside_a_frame():
    """steps 3 and 4 filter interleaved channels, each on its own; frame k of a batch equals the stage on frame k alone; a plane one
    sample past an aligned base, with other bytes around it in the frame, which stay as they were (`_run` checks them)."""
    rng = np.random.default_rng(40)
    m = case_frames(rng, 3, 37, 69, step=3)
    for interlaced in (False, True):
        whole = _check(m, 8, (4, 2), 5, interlaced)
        for k in range(3):
            assert np.array_equal(_run(m[k:k + 1], 8, (4, 2), 5, interlaced), whole[k:k + 1]), k
    _check(case_frames(rng, 2, 19, 21, step=1), 8, (4, 2), off=1, before=5, after=3)
    _check(case_frames(rng, 2, 19, 21, step=3, depth=12, above=True), 12, (4, 2), 5, True, off=2, before=6, after=2)
    _check(case_frames(rng, 1, 34, 260), 8, (15, 4), off=1, before=1)
    _check(case_frames(rng, 1, 35, 40, step=2), 8, (4, 2), interlaced=True, off=3)
    _check(case_frames(rng, 1, 35, 70, step=4), 8, (4, 2), before=4)
    _check(case_frames(rng, 1, 33, 67, step=4, depth=10, above=True), 10, (9, 3), 4, True, before=4)


def test_entries_refuse_bad_arguments():
    lib = _lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    out = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p, o = buf.data_ptr(), out.data_ptr()
    u8, u16 = lib.savsr_video_dering_u8, lib.savsr_video_dering_u16
    # (frames, n_frames, frame_bytes, plane_offset, rows, cols, step[, depth], interlaced, pri, sec, damping, out, out_frame_bytes, out_plane_offset)
    bad = [
        (u8, (0, 2, 64, 0, 8, 8, 1, 0, 4, 2, 5, o, 64, 0), "null pointer"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 4, 2, 5, 0, 64, 0), "null pointer"),
        (u8, (p, 0, 64, 0, 8, 8, 1, 0, 4, 2, 5, o, 64, 0), "n_frames >= 1"),
        (u8, (p, 2, 64, 0, 0, 8, 1, 0, 4, 2, 5, o, 64, 0), "rows >= 1"),
        (u8, (p, 2, 64, 0, 8, 0, 1, 0, 4, 2, 5, o, 64, 0), "at least one sample"),
        (u8, (p, 2, 64, 0, 8, 8, 0, 0, 4, 2, 5, o, 64, 0), "step 1 .. 4"),
        (u8, (p, 2, 64, 0, 8, 8, 5, 0, 4, 2, 5, o, 64, 0), "step 1 .. 4"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 2, 4, 2, 5, o, 64, 0), "interlaced 0 or 1"),
        (u8, (p, 2, 64, 0, 8, 8, 1, -1, 4, 2, 5, o, 64, 0), "interlaced 0 or 1"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 16, 2, 5, o, 64, 0), "pri a multiple"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, -1, 2, 5, o, 64, 0), "pri a multiple"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 4, 5, 5, o, 64, 0), "sec a multiple"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 4, -1, 5, o, 64, 0), "sec a multiple"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 4, 2, 2, o, 64, 0), "damping 3 .. 6"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 4, 2, 7, o, 64, 0), "damping 3 .. 6"),
        (u8, (p, 2, 63, 0, 8, 8, 1, 0, 4, 2, 5, o, 64, 0), "frame_bytes smaller"),
        (u8, (p, 2, 64, 0, 8, 4, 3, 0, 4, 2, 5, o, 64, 0), "frame_bytes smaller"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 4, 2, 5, o, 64, 1), "out_frame_bytes smaller"),
        (u8, (p, 2, 64, -1, 8, 8, 1, 0, 4, 2, 5, o, 64, 0), "plane offsets >= 0"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 4, 2, 5, p + 64, 64, 0), "the source frames and the output overlap"),
        (u16, (p, 2, 128, 0, 8, 8, 1, 8, 0, 4, 2, 5, o, 128, 0), "depth 10 or 12 (8 bits: savsr_video_dering_u8)"),
        (u16, (p + 1, 2, 128, 0, 8, 8, 1, 10, 0, 16, 8, 5, o, 128, 0), "2-byte aligned"),
        (u16, (p, 2, 130, 1, 8, 8, 1, 10, 0, 16, 8, 5, o, 128, 0), "2-byte aligned"),
        (u16, (p, 2, 128, 0, 8, 8, 1, 10, 0, 16, 8, 5, o + 1, 128, 0), "2-byte aligned"),
        (u16, (p, 2, 127, 0, 8, 8, 1, 10, 0, 16, 8, 5, o, 128, 0), "frame_bytes smaller"),
        (u16, (p, 2, 128, 0, 8, 8, 1, 10, 0, 18, 8, 5, o, 128, 0), "pri a multiple"),
        (u16, (p, 2, 128, 0, 8, 8, 1, 10, 0, 64, 8, 5, o, 128, 0), "pri a multiple"),
        (u16, (p, 2, 128, 0, 8, 8, 1, 12, 0, 64, 40, 5, o, 128, 0), "sec a multiple"),
        (u16, (p, 2, 128, 0, 8, 8, 1, 12, 0, 64, 80, 5, o, 128, 0), "sec a multiple"),
    ]
    for fn, args, words in bad:
        assert fn(*args, None) == -1, (fn.__name__, args)          # SAVSR_E_ARG
        msg = lib.savsr_last_error().decode()
        assert words in msg and fn.__name__[len("savsr_"):] in msg, (fn.__name__, args, msg)
    torch.cuda.synchronize()
    assert not out.any()                                             # refused before the device is touched: no launch left behind


# ---------------------------------------------------------------------------------------------------------------------- frames
def _planar(rng, n, h, w, depth, layout):
    sizes = [(h, w)] + ([] if layout == "400" else [yuv.chroma_hw(h, w, layout)] * 2)
    frames = np.concatenate([as_bytes(case_frames(rng, n, *hw, depth=depth)) for hw in sizes], 1)
    assert frames.shape[1] == yuv.frame_bytes(h, w, depth, layout)
    return np.ascontiguousarray(frames)


def test_dering_video_of_every_frame_kind():
    rng = np.random.default_rng(50)
    for c in (1, 3):
        v = case_frames(rng, 2, 19, 27, step=c)
        got = savsr_amd.dering_video(torch.from_numpy(v))
        assert got.device.type == "cuda" and got.dtype == torch.uint8 and got.shape == v.shape
        assert np.array_equal(got.cpu().numpy(), dering_frames(v)) and not np.array_equal(got.cpu().numpy(), v), c
        got = savsr_amd.dering_video(torch.from_numpy(v).to(DEV), strength=(9, 3), damping=4, interlaced=True)
        assert np.array_equal(got.cpu().numpy(), dering_frames(v, strength=(9, 3), damping=4, interlaced=True)), c
    for fmt, layout, depth, (h, w) in (("i420", "420", 8, (19, 37)), ("i422", "422", 8, (18, 36)), ("i444", "444", 8, (17, 18)),
                                       ("y400", "400", 8, (9, 33)), ("i420", "420", 10, (19, 37)), ("i444", "444", 12, (12, 18))):
        frames = _planar(rng, 2, h, w, depth, layout)
        for cs in (None, (12, 4)):
            for interlaced in (False, True):
                got = savsr_amd.dering_video(torch.from_numpy(frames), fmt, (h, w), depth, (4, 2), cs, 5, interlaced)
                want = dering_frames(frames, fmt, (h, w), depth, (4, 2), cs, 5, interlaced)
                assert np.array_equal(got.cpu().numpy(), want), (fmt, depth, h, w, cs, interlaced)
        if layout != "400":          # the chroma strength reaches the chroma planes alone
            ysz = h * w * (2 if depth > 8 else 1)
            a, b = dering_frames(frames, fmt, (h, w), depth, (4, 2), None), dering_frames(frames, fmt, (h, w), depth, (4, 2), (0, 0))
            assert np.array_equal(a[:, :ysz], b[:, :ysz]) and not np.array_equal(a[:, ysz:], b[:, ysz:])
    assert savsr_amd.dering_video(torch.zeros(0, 8, 8, 3, dtype=torch.uint8)).shape == (0, 8, 8, 3)
    with pytest.raises(ValueError, match="float frames have no integer samples to dering"):
        savsr_amd.dering_video(torch.zeros(3, 3, 4, 4, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------- the properties
H = W = 16
N = 12
KW = dict(dering="cdef", dering_strength=(9, 3), dering_damping=4)
ST = dict(strength=(9, 3), damping=4)
DKW = dict(deblock="strong", deblock_block=4, deblock_strength=(40, 20))
DST = dict(block=4, mode="strong", strength=(40, 20))


def _ringy(seed, n=N, h=H, w=W, c=3):
    rng = np.random.default_rng(seed)
    v = case_frames(rng, n, h, w, step=c).astype(np.int64)
    v += (np.arange(n) * 3)[:, None, None, None]          # the frames differ, so a wrong frame order shows
    return torch.from_numpy(np.clip(v, 0, 255).astype(np.uint8))


def test_property_plain_and_with_cuts(net3):
    v = _ringy(60)
    clean = savsr_amd.dering_video(v, **ST)
    assert not torch.equal(clean.cpu(), v) and not torch.equal(clean, savsr_amd.dering_video(v, **ST, interlaced=True))
    want = net3.upscale_video(clean, scale=2, out="uint8")
    got = net3.upscale_video(v, scale=2, out="uint8", **KW)
    assert got.shape == want.shape and torch.equal(got, want)
    assert not torch.equal(got, net3.upscale_video(v, scale=2, out="uint8"))
    assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", dering=None), net3.upscale_video(v, scale=2, out="uint8"))
    assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", dering="cdef"),
                       net3.upscale_video(savsr_amd.dering_video(v), scale=2, out="uint8"))
    # cuts="auto" scores the filtered frames
    assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", cuts="auto", scene_threshold=1.0, **KW),
                       net3.upscale_video(clean, scale=2, out="uint8", cuts="auto", scene_threshold=1.0))


def test_property_behind_the_deblocker(net3):
    """deblock= first, dering= on its result; the two stages swapped by hand give other bytes."""
    v = _ringy(66)
    both = savsr_amd.dering_video(savsr_amd.deblock_video(v, **DST), **ST)
    swapped = savsr_amd.deblock_video(savsr_amd.dering_video(v, **ST), **DST)
    assert not torch.equal(both, swapped)
    got = net3.upscale_video(v, scale=2, out="uint8", **DKW, **KW)
    assert torch.equal(got, net3.upscale_video(both, scale=2, out="uint8"))
    assert not torch.equal(got, net3.upscale_video(swapped, scale=2, out="uint8"))
    # field-wise exactly when the deblocker is
    both = savsr_amd.dering_video(savsr_amd.deblock_video(v, **DST, interlaced=True), **ST, interlaced=True)
    assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", fields="bff", **DKW, **KW), net3.upscale_video(both, scale=2, out="uint8", fields="bff"))


def test_property_in_front_of_fields_and_pulldown(net3):
    """fields= and pulldown= make the stage field-wise, and it runs on the source frames, in front of either."""
    v = _ringy(61, n=10)
    by_field = savsr_amd.dering_video(v, **ST, interlaced=True)
    got = net3.upscale_video(v, scale=2, out="uint8", fields="tff", **KW)
    assert got.shape[0] == 20 and torch.equal(got, net3.upscale_video(by_field, scale=2, out="uint8", fields="tff"))
    assert not torch.equal(got, net3.upscale_video(savsr_amd.dering_video(v, **ST), scale=2, out="uint8", fields="tff"))
    got = net3.upscale_video(v, scale=2, out="uint8", pulldown="tff", **KW)
    assert got.shape[0] == 8 and torch.equal(got, net3.upscale_video(by_field, scale=2, out="uint8", pulldown="tff"))


def test_property_in_front_of_the_crop_and_the_denoisers(net3):
    """crop= crops the filtered frames (the 8 x 8 grid is the full frame's: cropping first and filtering the crop gives other bytes), and
    the denoisers see the filtered frames."""
    v = _ringy(62)
    rect = (2, 6, 8, 10)
    clean = savsr_amd.dering_video(v, **ST)
    assert not torch.equal(clean[:, 2:10, 6:16].cpu(), savsr_amd.dering_video(v[:, 2:10, 6:16].contiguous(), **ST).cpu())
    more = dict(spatial_denoise="nlm", spatial_patch=1, spatial_search=2, denoise="ata", denoise_radius=2)
    for bars in ("drop", "keep"):
        want = net3.upscale_video(clean, scale=2, out="uint8", crop=rect, bars=bars, **more)
        assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", crop=rect, bars=bars, **more, **KW), want), bars
    assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", crop="auto", **KW), net3.upscale_video(clean, scale=2, out="uint8", crop="auto"))


def test_property_with_scan_detect(net3):
    """The detector reads the unfiltered frames; an interlaced verdict makes the stage field-wise."""
    v = torch.from_numpy(packed_case("interlaced", "tff", H, W, motion=(2, 1), n=N))
    verdict = savsr_amd.detect_scan(v)
    assert verdict.scan == "interlaced" and verdict.kwargs() == {"fields": "tff"}
    clean = savsr_amd.dering_video(v, **ST, interlaced=verdict.scan in ("interlaced", "telecine"))
    assert not torch.equal(clean.cpu(), v)
    want = net3.upscale_video(clean, scale=2, out="uint8", **verdict.kwargs())
    got = net3.upscale_video(v, scale=2, out="uint8", scan="detect", **KW)
    assert got.shape[0] == 2 * N and torch.equal(got, want)
    p = torch.from_numpy(packed_case("progressive", None, H, W, motion=(2, 1), n=N))
    assert savsr_amd.detect_scan(p).kwargs() == {}
    assert torch.equal(net3.upscale_video(p, scale=2, out="uint8", scan="detect", **KW),
                       net3.upscale_video(savsr_amd.dering_video(p, **ST), scale=2, out="uint8"))


def test_property_planar_with_a_chroma_strength(net3):
    rng = np.random.default_rng(63)
    frames = torch.from_numpy(_planar(rng, N, H, W, 8, "420"))
    fmt = dict(pixel_format="i420", size=(H, W), out="i420")
    clean = savsr_amd.dering_video(frames, "i420", (H, W), 8, (9, 3), (15, 4), 4)
    assert not torch.equal(clean, savsr_amd.dering_video(frames, "i420", (H, W), 8, (9, 3), None, 4))
    want = net3.upscale_video(clean, scale=2, **fmt)
    assert torch.equal(net3.upscale_video(frames, scale=2, **fmt, dering_chroma_strength=(15, 4), **KW), want)


@pytest.mark.parametrize("chunk", [1, 5, 12])
def test_video_upscaler_under_any_chunking(net3, chunk):
    from savsr_amd import VideoUpscaler
    v = _ringy(64)
    for extra in ({}, dict(crop=(2, 4, 8, 12), bars="drop", cuts="auto", scene_threshold=1.0, **DKW), dict(fields="tff"),
                  dict(pulldown="bff", denoise="ata", denoise_radius=2)):
        whole = net3.upscale_video(v, scale=2, out="uint8", **KW, **extra)
        up = VideoUpscaler(net3, 2, out="uint8", **KW, **extra)
        parts = [up.push(v[a:a + chunk]) for a in range(0, N, chunk)] + [up.finish()]
        assert torch.equal(torch.cat(parts, 0), whole), extra


def test_refused_arguments_leave_no_launch_behind(net3):
    from savsr_amd import VideoUpscaler
    v = _ringy(65)
    lib = _lib()
    assert lib.savsr_video_dering_u8(0, 1, 1, 0, 1, 1, 1, 0, 4, 2, 5, 0, 1, 0, None) == -1          # a known last error to compare against
    before = lib.savsr_last_error()
    for call in (lambda **kw: net3.upscale_video(v, scale=2, out="uint8", **kw), lambda **kw: VideoUpscaler(net3, 2, out="uint8", **kw)):
        for kw, words in ((dict(dering="strong"), "dering = 'strong'"), (dict(dering_strength=(4, 3)), "goes with dering="),
                          (dict(dering_chroma_strength=(4, 2)), "goes with dering="), (dict(dering_damping=4), "goes with dering="),
                          (dict(dering="cdef", dering_strength=(16, 2)), r"dering_strength = \(16, 2\)"),
                          (dict(dering="cdef", dering_strength=(4, 5)), r"dering_strength = \(4, 5\)"),
                          (dict(dering="cdef", dering_strength=(4.0, 2)), r"dering_strength = \(4.0, 2\)"),
                          (dict(dering="cdef", dering_strength=4), "dering_strength = 4"),
                          (dict(dering="cdef", dering_chroma_strength=(-1, 2)), r"dering_chroma_strength = \(-1, 2\)"),
                          (dict(dering="cdef", dering_damping=2), "dering_damping = 2"),
                          (dict(dering="cdef", dering_damping=7), "dering_damping = 7")):
            with pytest.raises(ValueError, match=words):
                call(**kw)
    with pytest.raises(ValueError, match="float frames have no integer samples to dering"):
        net3.upscale_video(torch.zeros(8, 3, H, W, device=DEV), scale=2, dering="cdef")
    up = VideoUpscaler(net3, 2, dering="cdef")
    with pytest.raises(ValueError, match="float frames have no integer samples to dering"):
        up.push(torch.zeros(8, 3, H, W, device=DEV))
    assert lib.savsr_last_error() == before and b"video_dering_u8: null pointer" in before


# ---------------------------------------------------------------------------------------------------------------------- the CLI
def _y4m_bytes(sr, w, h, fps, tag, lr):
    g = io.BytesIO()
    y4m.Y4MWriter(g, w, h, fps, tag, y4m.scaled_aspect((1, 1), lr, (h, w))).write(sr.cpu().numpy())
    return g.getvalue()


def test_cli_dering_on_a_y4m_file(net3, tmp_path, capsys):
    """--dering on a file whose content is interlaced: progressive as the file is tagged, field-wise behind --scan detect (whose first
    pass reads the unfiltered frames), behind --deblock, and --crop auto's first pass reads the filtered frames.  One line on stderr
    says which."""
    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    frames = planar_case("interlaced", "tff", H, W, motion=(2, 1), n=8)
    f = io.BytesIO()
    y4m.Y4MWriter(f, W, H, (25, 1), "p", (1, 1)).write(frames)
    src, ckpt = tmp_path / "lr.y4m", tmp_path / "net.pth"
    src.write_bytes(f.getvalue())
    sio.save_network(net3, str(ckpt))
    base = ["-i", str(src), "--scale", "2", "--checkpoint", str(ckpt), "--chunk", "3", "--dering", "cdef", "--dering-strength", "9,3",
            "--dering-chroma-strength", "15,4", "--dering-damping", "4"]
    fmt = dict(scale=2, out="i420", pixel_format="i420", size=(H, W), dering_chroma_strength=(15, 4), **KW)
    v = torch.from_numpy(frames)
    plain, scan, crop = tmp_path / "plain.y4m", tmp_path / "scan.y4m", tmp_path / "crop.y4m"
    assert main(base + ["-o", str(plain)]) == 0
    assert "--dering cdef: strength 9,3, chroma strength 15,4, damping 4 (8-bit code units; not validated on footage), progressive" in capsys.readouterr().err
    assert plain.read_bytes() == _y4m_bytes(net3.upscale_video(v, **fmt), 2 * W, 2 * H, (25, 1), "p", (H, W))
    assert plain.read_bytes() != _y4m_bytes(net3.upscale_video(v, scale=2, out="i420", pixel_format="i420", size=(H, W)), 2 * W, 2 * H, (25, 1), "p", (H, W))
    assert main(base + ["-o", str(scan), "--scan", "detect", "--deblock", "strong", "--deblock-block", "4"]) == 0
    err = capsys.readouterr().err
    assert "--scan detect: interlaced, top field first: --fields tff" in err
    assert "damping 4 (8-bit code units; not validated on footage), field-wise (the fields as planes of their own)" in err
    want = net3.upscale_video(v, scan="detect", deblock="strong", deblock_block=4, **fmt)
    assert want.shape[0] == 16 and scan.read_bytes() == _y4m_bytes(want, 2 * W, 2 * H, (50, 1), "p", (H, W))
    assert main(base + ["-o", str(crop), "--crop", "auto"]) == 0
    assert crop.read_bytes() == _y4m_bytes(net3.upscale_video(v, crop="auto", **fmt), 2 * W, 2 * H, (25, 1), "p", (H, W))
