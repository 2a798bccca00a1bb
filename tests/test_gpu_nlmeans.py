"""GPU checks of the spatial denoiser: savsr_video_nlmeans_u8 / _u16 against the numpy specification bit for bit between guard bytes
(the shared generator and shapes of tests/nlmeans_cases.py: planes smaller than the halo, one tile plus a row and a column, two tiles
each way with a ragged rest; every patch x search; the divisor's range; every depth with samples above it; the largest numerator;
steps 1 and 3; 1 and 3 frames; a plane inside a frame at a misaligned base), the entries' refusals, `denoise_spatial` on every frame
kind, and the properties of upscale_video(spatial_denoise="nlm"): bit for bit the call on the filtered video, after the crop, behind
denoise= and fields=, and in VideoUpscaler under any chunking."""
import numpy as np
import pytest
import torch

import savsr_amd
from savsr_amd import active, yuv
from savsr_amd.nlmeans import divisor, nlm_frames, nlm_matrix
from savsr_amd.utils import synth
from tests.nlmeans_cases import DEPTHS, MAX_DIVISOR, PATCHES, SEARCHES, TINY, as_bytes, case_frames, one_tile_plus, two_tiles_ragged
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


def _run(m, depth=8, patch=3, search=7, div=441, off=0, before=0, after=0):
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
    lib, st = _lib(), torch.cuda.current_stream().cuda_stream
    head = (src.data_ptr() + off, n, fb, before, r, c, step)
    tail = (patch, search, div, dst.data_ptr() + off, fb, before, st)
    rc = lib.savsr_video_nlmeans_u16(*head, depth, *tail) if depth > 8 else lib.savsr_video_nlmeans_u8(*head, *tail)
    assert rc == 0, lib.savsr_last_error()
    got = dst.cpu().numpy()
    assert (got[:off] == POISON).all() and (got[off + n * fb:] == POISON).all()
    got = got[off:off + n * fb].reshape(n, fb)
    assert (got[:, :before] == POISON).all() and (got[:, before + plane.shape[1]:] == POISON).all()
    got = np.ascontiguousarray(got[:, before:before + plane.shape[1]])
    return got.view("<u2").reshape(m.shape) if depth > 8 else got.reshape(m.shape)


def _want(m, depth, patch, search, div):
    out = np.empty_like(m)
    for t in range(m.shape[0]):
        for ch in range(m.shape[3]):
            out[t, :, :, ch] = nlm_matrix(m[t, :, :, ch], depth, patch, search, div)
    return out


def _check(m, depth=8, patch=3, search=7, div=441, **place):
    got, want = _run(m, depth, patch, search, div, **place), _want(m, depth, patch, search, div)
    assert np.array_equal(got, want), (m.shape, depth, patch, search, div, place, np.argwhere(got != want)[:4].tolist())


# ---------------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("search", SEARCHES)
@pytest.mark.parametrize("patch", PATCHES)
def test_entries_equal_the_spec_at_every_patch_and_search(patch, search):
    """Planes smaller than the halo and one tile plus a row and a column (the second strip's first row, the second tile's first column),
    at the default divisor of the patch, at 8 and at 10 bits."""
    rng = np.random.default_rng(10 * patch + search)
    for r, c in TINY + (one_tile_plus(patch),):
        _check(case_frames(rng, 1, r, c), 8, patch, search, divisor(patch, 3.0))
    _check(case_frames(rng, 1, 17, 9, depth=10, above=True), 10, patch, search, divisor(patch, 3.0))


@pytest.mark.parametrize("patch", PATCHES)
def test_two_tiles_each_way_with_a_ragged_rest(patch):
    rng = np.random.default_rng(20 + patch)
    r, c = two_tiles_ragged(patch)
    _check(case_frames(rng, 1, r, c), 8, patch, 7 if patch == 3 else 3, divisor(patch, 3.0))


@pytest.mark.parametrize("depth", DEPTHS)
def test_every_depth_and_the_divisors_range(depth):
    """D = 1 (the identity wherever no two patches are equal), the default and the largest a caller can ask for (h = 32); 16-bit planes
    carry samples above 2^d - 1, which are read as 2^d - 1."""
    rng = np.random.default_rng(30 + depth)
    m = case_frames(rng, 1, 21, 70, depth=depth, above=True)
    for div in (1, divisor(3, 3.0), MAX_DIVISOR):
        _check(m, depth, 3, 7, div)
    _check(m, depth, 1, 2, 9 * 32 * 32)


def test_the_largest_numerator_and_a_plane_of_ffff():
    """A constant 4095 plane at depth 12, S = 7: where all 225 candidates lie inside the plane the numerator is 225 * 4096 * 4095 =
    3 773 952 000, the largest there is, and with the rounding term still below 2^32.  A plane of 0xFFFF is read as 4095 throughout."""
    m = np.full((1, 17, 20, 1), 4095, np.uint16)
    out, counts = nlm_matrix(m[0, :, :, 0], 12, 3, 7, 441, True)
    assert counts["sum_max"] == 3773952000 == 225 * 4096 * 4095 and (out == 4095).all()
    assert np.array_equal(_run(m, 12, 3, 7, 441), m)
    ffff = np.full((1, 17, 20, 1), 0xFFFF, np.uint16)
    for depth in (10, 12):
        assert (_run(ffff, depth, 3, 7, 441) == (1 << depth) - 1).all()
    assert np.array_equal(_run(np.full((1, 70, 70, 1), 255, np.uint8), 8, 3, 7, 1), np.full((1, 70, 70, 1), 255, np.uint8))


def test_steps_frames_and_a_misaligned_plane_inside_a_frame():
    """step 3 filters three interleaved channels, each on its own; frame k of a batch equals the stage on frame k alone; a plane one
    sample past an aligned base, with other bytes around it in the frame, which stay as they were (`_run` checks them)."""
    rng = np.random.default_rng(40)
    m = case_frames(rng, 3, 19, 23, step=3)
    _check(m, 8, 2, 3, divisor(2, 3.0))
    whole = _run(m, 8, 3, 7, 441)
    for k in range(3):
        assert np.array_equal(_run(m[k:k + 1], 8, 3, 7, 441), whole[k:k + 1]), k
    assert np.array_equal(whole, _want(m, 8, 3, 7, 441))
    _check(case_frames(rng, 2, 9, 11, step=1), 8, 3, 7, 441, off=1, before=5, after=3)
    _check(case_frames(rng, 2, 9, 11, step=3, depth=12, above=True), 12, 3, 5, 441, off=2, before=6, after=2)
    _check(case_frames(rng, 1, 66, 60), 8, 3, 7, 441, off=1, before=1)


def test_entries_refuse_bad_arguments():
    lib = _lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    out = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p, o = buf.data_ptr(), out.data_ptr()
    u8, u16 = lib.savsr_video_nlmeans_u8, lib.savsr_video_nlmeans_u16
    # (frames, n_frames, frame_bytes, plane_offset, rows, cols, step[, depth], patch, search, divisor, out, out_frame_bytes, out_plane_offset)
    bad = [
        (u8, (0, 2, 64, 0, 8, 8, 1, 3, 7, 441, o, 64, 0), "null pointer"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 3, 7, 441, 0, 64, 0), "null pointer"),
        (u8, (p, 0, 64, 0, 8, 8, 1, 3, 7, 441, o, 64, 0), "n_frames >= 1"),
        (u8, (p, 2, 64, 0, 0, 8, 1, 3, 7, 441, o, 64, 0), "rows >= 1"),
        (u8, (p, 2, 64, 0, 8, 0, 1, 3, 7, 441, o, 64, 0), "at least one sample"),
        (u8, (p, 2, 64, 0, 8, 8, 0, 3, 7, 441, o, 64, 0), "step 1 .. 4"),
        (u8, (p, 2, 64, 0, 8, 8, 5, 3, 7, 441, o, 64, 0), "step 1 .. 4"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 7, 441, o, 64, 0), "patch 1 .. 3"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 4, 7, 441, o, 64, 0), "patch 1 .. 3"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 3, 0, 441, o, 64, 0), "search 1 .. 7"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 3, 8, 441, o, 64, 0), "search 1 .. 7"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 3, 7, 0, o, 64, 0), "divisor 1 .. 65536"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 3, 7, 65537, o, 64, 0), "divisor 1 .. 65536"),
        (u8, (p, 2, 63, 0, 8, 8, 1, 3, 7, 441, o, 64, 0), "frame_bytes smaller"),
        (u8, (p, 2, 64, 0, 8, 4, 3, 3, 7, 441, o, 64, 0), "frame_bytes smaller"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 3, 7, 441, o, 64, 1), "out_frame_bytes smaller"),
        (u8, (p, 2, 64, -1, 8, 8, 1, 3, 7, 441, o, 64, 0), "plane offsets >= 0"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 3, 7, 441, p + 64, 64, 0), "the source frames and the output overlap"),
        (u16, (p, 2, 128, 0, 8, 8, 1, 8, 3, 7, 441, o, 128, 0), "depth 10 or 12 (8 bits: savsr_video_nlmeans_u8)"),
        (u16, (p + 1, 2, 128, 0, 8, 8, 1, 10, 3, 7, 441, o, 128, 0), "2-byte aligned"),
        (u16, (p, 2, 130, 1, 8, 8, 1, 10, 3, 7, 441, o, 128, 0), "2-byte aligned"),
        (u16, (p, 2, 128, 0, 8, 8, 1, 10, 3, 7, 441, o + 1, 128, 0), "2-byte aligned"),
        (u16, (p, 2, 127, 0, 8, 8, 1, 10, 3, 7, 441, o, 128, 0), "frame_bytes smaller"),
        (u16, (p, 2, 128, 0, 8, 8, 1, 12, 3, 9, 441, o, 128, 0), "search 1 .. 7"),
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


def test_denoise_spatial_of_every_frame_kind():
    rng = np.random.default_rng(50)
    for c in (1, 3):
        v = case_frames(rng, 2, 9, 13, step=c)
        got = savsr_amd.denoise_spatial(torch.from_numpy(v))
        assert got.device.type == "cuda" and got.dtype == torch.uint8 and got.shape == v.shape
        assert np.array_equal(got.cpu().numpy(), nlm_frames(v)), c
        got = savsr_amd.denoise_spatial(torch.from_numpy(v).to(DEV), patch=1, search=2, strength=6)
        assert np.array_equal(got.cpu().numpy(), nlm_frames(v, patch=1, search=2, strength=6)), c
    for fmt, layout, depth, (h, w) in (("i420", "420", 8, (7, 9)), ("i422", "422", 8, (8, 16)), ("i444", "444", 8, (6, 8)),
                                       ("y400", "400", 8, (5, 33)), ("i420", "420", 10, (7, 9)), ("i444", "444", 12, (4, 8))):
        frames = _planar(rng, 2, h, w, depth, layout)
        for cs in (None, 1.0):
            got = savsr_amd.denoise_spatial(torch.from_numpy(frames), fmt, (h, w), depth, 3, 7, 3.0, cs)
            want = nlm_frames(frames, fmt, (h, w), depth, 3, 7, 3.0, cs)
            assert np.array_equal(got.cpu().numpy(), want), (fmt, depth, h, w, cs)
        if layout != "400":          # the chroma strength reaches the chroma planes alone
            ysz = h * w * (2 if depth > 8 else 1)
            a, b = nlm_frames(frames, fmt, (h, w), depth, 3, 7, 3.0, None), nlm_frames(frames, fmt, (h, w), depth, 3, 7, 3.0, 32)
            assert np.array_equal(a[:, :ysz], b[:, :ysz]) and not np.array_equal(a[:, ysz:], b[:, ysz:])
    with pytest.raises(ValueError, match="float frames have no integer samples to denoise"):
        savsr_amd.denoise_spatial(torch.zeros(3, 3, 4, 4, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------- the properties
H = W = 16
N = 12
KW = dict(spatial_denoise="nlm", spatial_patch=2, spatial_search=3, spatial_strength=4.0)
ST = dict(patch=2, search=3, strength=4.0)


def _noisy(seed, n=N, h=H, w=W, c=3):
    rng = np.random.default_rng(seed)
    v = case_frames(rng, n, h, w, step=c).astype(np.int64)
    v += (np.arange(n) * 3)[:, None, None, None]          # the frames differ, so a wrong frame order shows
    return torch.from_numpy(np.clip(v, 0, 255).astype(np.uint8))


def test_property_without_a_crop_and_with_cuts(net3):
    v = _noisy(60)
    clean = savsr_amd.denoise_spatial(v, **ST)
    assert not torch.equal(clean.cpu(), v)
    want = net3.upscale_video(clean, scale=2, out="uint8")
    got = net3.upscale_video(v, scale=2, out="uint8", **KW)
    assert got.shape == want.shape and torch.equal(got, want)
    assert not torch.equal(got, net3.upscale_video(v, scale=2, out="uint8"))
    assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", spatial_denoise=None), net3.upscale_video(v, scale=2, out="uint8"))
    # cuts="auto" scores the filtered frames
    assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", cuts="auto", scene_threshold=1.0, **KW),
                       net3.upscale_video(clean, scale=2, out="uint8", cuts="auto", scene_threshold=1.0))


def test_property_after_the_crop(net3):
    """bars="drop": the call on the filtered crop; bars="keep": the picture inside the bars is those bytes.  The rule does not commute
    with a crop: filtering first and cropping afterwards gives other bytes."""
    v = _noisy(61)
    rect = (2, 4, 8, 12)
    cropped = torch.from_numpy(active.crop_frames(v.numpy(), rect))
    clean = savsr_amd.denoise_spatial(cropped, **ST)
    assert not torch.equal(clean, savsr_amd.denoise_spatial(v, **ST)[:, 2:10, 4:16])
    want = net3.upscale_video(clean, scale=2, out="uint8")
    got = net3.upscale_video(v, scale=2, out="uint8", crop=rect, bars="drop", **KW)
    assert torch.equal(got, want)
    kept = net3.upscale_video(v, scale=2, out="uint8", crop=rect, bars="keep", **KW)
    assert kept.shape[1:3] == (2 * H, 2 * W) and torch.equal(kept[:, 4:20, 8:32], want)


def test_property_behind_denoise_and_fields(net3):
    v = _noisy(62, n=10)
    temporal = savsr_amd.denoise_video(v, radius=2, strength=(4, 9))
    want = net3.upscale_video(savsr_amd.denoise_spatial(temporal, **ST), scale=2, out="uint8")
    assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", denoise="ata", denoise_radius=2, **KW), want)
    prog = savsr_amd.deinterlace(v, "tff")
    want = net3.upscale_video(savsr_amd.denoise_spatial(prog, **ST), scale=2, out="uint8")
    got = net3.upscale_video(v, scale=2, out="uint8", fields="tff", **KW)
    assert got.shape[0] == 20 and torch.equal(got, want)


def test_property_planar(net3):
    rng = np.random.default_rng(63)
    frames = torch.from_numpy(_planar(rng, N, H, W, 8, "420"))
    fmt = dict(pixel_format="i420", size=(H, W), out="i420")
    clean = savsr_amd.denoise_spatial(frames, "i420", (H, W), 8, 2, 3, 4.0, 2.0)
    want = net3.upscale_video(clean, scale=2, **fmt)
    assert torch.equal(net3.upscale_video(frames, scale=2, **fmt, spatial_chroma_strength=2.0, **KW), want)


@pytest.mark.parametrize("chunk", [1, 5, 12])
def test_video_upscaler_under_any_chunking(net3, chunk):
    from savsr_amd import VideoUpscaler
    v = _noisy(64)
    for extra in ({}, dict(crop=(2, 4, 8, 12), bars="drop", cuts="auto", scene_threshold=1.0), dict(denoise="ata", denoise_radius=2)):
        whole = net3.upscale_video(v, scale=2, out="uint8", **KW, **extra)
        up = VideoUpscaler(net3, 2, out="uint8", **KW, **extra)
        parts = [up.push(v[a:a + chunk]) for a in range(0, N, chunk)] + [up.finish()]
        assert torch.equal(torch.cat(parts, 0), whole), extra


def test_refused_arguments_leave_no_launch_behind(net3):
    from savsr_amd import VideoUpscaler
    v = _noisy(65)
    lib = _lib()
    assert lib.savsr_video_nlmeans_u8(0, 1, 1, 0, 1, 1, 1, 3, 7, 441, 0, 1, 0, None) == -1          # a known last error to compare against
    before = lib.savsr_last_error()
    for call in (lambda **kw: net3.upscale_video(v, scale=2, out="uint8", **kw), lambda **kw: VideoUpscaler(net3, 2, out="uint8", **kw)):
        for kw, words in ((dict(spatial_denoise="nlmeans"), "spatial_denoise = 'nlmeans'"), (dict(spatial_patch=2), "goes with spatial_denoise="),
                          (dict(spatial_denoise="nlm", spatial_patch=4), "spatial_patch = 4"),
                          (dict(spatial_denoise="nlm", spatial_search=8), "spatial_search = 8"),
                          (dict(spatial_denoise="nlm", spatial_strength=0), "spatial_strength = 0"),
                          (dict(spatial_denoise="nlm", spatial_strength=True), "spatial_strength = True"),
                          (dict(denoise="nlmeans"), "denoise = 'nlmeans'")):
            with pytest.raises(ValueError, match=words):
                call(**kw)
    with pytest.raises(ValueError, match="float frames have no integer samples to denoise"):
        net3.upscale_video(torch.zeros(8, 3, H, W, device=DEV), scale=2, spatial_denoise="nlm")
    assert lib.savsr_last_error() == before and b"video_nlmeans_u8: null pointer" in before
