"""GPU checks of the temporal denoiser: savsr_video_denoise_u8 / _u16 against the numpy specification bit for bit between guard bytes
(the shared generator and matrices of tests/denoise_cases.py, both forms of the kernels, aligned and misaligned bases, planes inside
frames, every radius and depth, videos shorter than the radius, sub-ranges with their taps outside), the entries' refusals,
`denoise_video` on every frame kind, TemporalDenoiser under any chunking, and the property of upscale_video(denoise="ata"): bit for bit
the call on the denoised video, also behind fields=, pulldown= and surface= and in front of crop=."""
import numpy as np
import pytest
import torch

import savsr_amd
from savsr_amd import yuv
from savsr_amd.denoise import denoise_frames, denoise_matrix
from savsr_amd.surface import Surface
from savsr_amd.utils import synth
from tests.denoise_cases import DEPTHS, MATRICES, RADII, STRENGTH, TIGHT, as_bytes, lengths_for, walk_video
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


def _run(mats, depth=8, radius=4, strength=STRENGTH, rng=None, off=0, before=0, after=0):
    """One entry on the matrices [N, R, C] as the plane `before` bytes into frames of before + plane + after bytes, the first frame `off`
    bytes past a 256-byte aligned allocation; frames [rng) (default: all).  The output frames have the same layout, are poisoned first
    and are followed by guard bytes: nothing outside the planes is written.  Returns [hi - lo, R, C]."""
    n, r, c = mats.shape
    lo, hi = rng or (0, n)
    plane = as_bytes(mats)
    fb = before + plane.shape[1] + after
    host = np.full((n, fb), 0x3C, np.uint8)
    host[:, before:before + plane.shape[1]] = plane
    src = torch.empty(n * fb + off + 64, dtype=torch.uint8, device=DEV)
    assert src.data_ptr() % 256 == 0
    src[off:off + n * fb].copy_(torch.from_numpy(host).reshape(-1))
    no = hi - lo
    dst = torch.full((no * fb + off + 64,), POISON, dtype=torch.uint8, device=DEV)
    assert dst.data_ptr() % 256 == 0
    lib, st = _lib(), torch.cuda.current_stream().cuda_stream
    head = (src.data_ptr() + off, n, fb, before, r, c)
    tail = (radius, strength[0], strength[1], lo, hi, dst.data_ptr() + off, fb, before, st)
    rc = lib.savsr_video_denoise_u16(*head, depth, *tail) if depth > 8 else lib.savsr_video_denoise_u8(*head, *tail)
    assert rc == 0, lib.savsr_last_error()
    got = dst.cpu().numpy()
    assert (got[:off] == POISON).all() and (got[off + no * fb:] == POISON).all()
    got = got[off:off + no * fb].reshape(no, fb)
    assert (got[:, :before] == POISON).all() and (got[:, before + plane.shape[1]:] == POISON).all()
    got = got[:, before:before + plane.shape[1]]
    return np.ascontiguousarray(got).view("<u2").reshape(no, r, c) if depth > 8 else got.reshape(no, r, c)


def _is_vec(r, c, depth, off=0, before=0, after=0):
    """Whether the launch takes the vector form: plane pointers, frame strides and the plane's bytes are multiples of 16."""
    plane = r * c * (2 if depth > 8 else 1)
    return (off + before) % 16 == 0 and (before + plane + after) % 16 == 0 and plane % 16 == 0


# ---------------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("radius", RADII)
def test_entries_equal_the_spec(radius, depth):
    """Every matrix x video length, from an aligned base (planes of 128, 816 and 432 bytes take the vector form at 8 bits, the others the
    one-sample form) and one sample off (the one-sample form for all): both equal the specification, so they equal each other."""
    rng = np.random.default_rng(100 * radius + depth)
    step = 2 if depth > 8 else 1
    forms = set()
    for r, c in MATRICES:
        for n in lengths_for(radius):
            m = walk_video(rng, n, r, c, depth)
            if depth > 8:
                m[:, ::2, ::5] = 60000          # codes above 2^d - 1 are read as 2^d - 1
            want = denoise_matrix(m, radius, *STRENGTH, depth)
            for off in (0, step):
                forms.add(_is_vec(r, c, depth, off))
                got = _run(m, depth, radius, off=off)
                assert np.array_equal(got, want), (r, c, n, off, np.argwhere(got != want)[:4])
            if radius <= 2:                     # the B stop at small radii
                assert np.array_equal(_run(m, depth, radius, TIGHT), denoise_matrix(m, radius, *TIGHT, depth)), (r, c, n)
    assert forms == {True, False}


@pytest.mark.parametrize("depth", DEPTHS)
def test_the_top_of_the_range_and_every_divisor(depth):
    """All samples 2^d - 1 at radius 16: n frames give k = n up to 17, and 38 frames k = 17 .. 33, in both forms."""
    top = (1 << depth) - 1
    for n in list(range(1, 18)) + [38]:
        for shape in ((2, 32), (1, 5)):
            m = np.full((n,) + shape, top, np.uint8 if depth == 8 else np.uint16)
            assert np.array_equal(_run(m, depth, 16, (255, 255)), m), (n, shape)


def test_ranges_with_their_taps_outside_and_planes_inside_frames():
    rng = np.random.default_rng(7)
    for depth, places in ((8, ((0, 0, True), (16, 32, True), (32, 0, True), (5, 3, False), (16, 8, False))),
                          (12, ((0, 0, True), (16, 16, True), (6, 10, False), (2, 4, False)))):
        for radius in (2, 4):
            n = 2 * radius + 6
            for r, c in ((4, 32), (9, 48), (5, 33)):
                m = walk_video(rng, n, r, c, depth)
                want = denoise_matrix(m, radius, *STRENGTH, depth)
                for before, after, vec in places:
                    if (r, c) != (5, 33):
                        assert _is_vec(r, c, depth, 0, before, after) == vec
                    for lo, hi in ((0, 1), (radius, radius + 3), (n - 2, n), (1, n - 1)):
                        got = _run(m, depth, radius, rng=(lo, hi), before=before, after=after)
                        assert np.array_equal(got, want[lo:hi]), (depth, radius, r, c, before, after, lo, hi)
    m = walk_video(rng, 8, 4, 32)
    assert not np.array_equal(_run(m[3:4], 8, 2), denoise_matrix(m, 2, *STRENGTH)[3:4])          # a range without its context is another video


def test_entries_refuse_bad_arguments():
    lib = _lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    out = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p, o = buf.data_ptr(), out.data_ptr()
    u8, u16 = lib.savsr_video_denoise_u8, lib.savsr_video_denoise_u16
    # (frames, n_frames, frame_bytes, plane_offset, rows, row_bytes | cols[, depth], radius, thr_a, thr_b, from, to, out, out_frame_bytes, out_plane_offset)
    bad = [
        (u8, (0, 2, 64, 0, 8, 8, 4, 4, 9, 0, 2, o, 64, 0), "null pointer"),
        (u8, (p, 2, 64, 0, 8, 8, 4, 4, 9, 0, 2, 0, 64, 0), "null pointer"),
        (u8, (p, 0, 64, 0, 8, 8, 4, 4, 9, 0, 0, o, 64, 0), "n_frames >= 1"),
        (u8, (p, 2, 64, 0, 0, 8, 4, 4, 9, 0, 2, o, 64, 0), "rows >= 1"),
        (u8, (p, 2, 64, 0, 8, 0, 4, 4, 9, 0, 2, o, 64, 0), "at least one sample"),
        (u8, (p, 2, 64, 0, 8, 8, 0, 4, 9, 0, 2, o, 64, 0), "radius 1 .. 16"),
        (u8, (p, 2, 64, 0, 8, 8, 17, 4, 9, 0, 2, o, 64, 0), "radius 1 .. 16"),
        (u8, (p, 2, 64, 0, 8, 8, 4, 9, 4, 0, 2, o, 64, 0), "0 <= thr_a <= thr_b <= 255"),
        (u8, (p, 2, 64, 0, 8, 8, 4, -1, 4, 0, 2, o, 64, 0), "0 <= thr_a <= thr_b <= 255"),
        (u8, (p, 2, 64, 0, 8, 8, 4, 4, 256, 0, 2, o, 64, 0), "0 <= thr_a <= thr_b <= 255"),
        (u8, (p, 2, 64, 0, 8, 8, 4, 4, 9, -1, 2, o, 64, 0), "0 <= from < to <= n_frames"),
        (u8, (p, 2, 64, 0, 8, 8, 4, 4, 9, 0, 3, o, 64, 0), "0 <= from < to <= n_frames"),
        (u8, (p, 2, 64, 0, 8, 8, 4, 4, 9, 1, 1, o, 64, 0), "0 <= from < to <= n_frames"),
        (u8, (p, 2, 63, 0, 8, 8, 4, 4, 9, 0, 2, o, 64, 0), "frame_bytes smaller"),
        (u8, (p, 2, 64, 0, 8, 8, 4, 4, 9, 0, 2, o, 64, 1), "out_frame_bytes smaller"),
        (u8, (p, 2, 64, -1, 8, 8, 4, 4, 9, 0, 2, o, 64, 0), "plane offsets >= 0"),
        (u8, (p, 2, 64, 0, 8, 8, 4, 4, 9, 0, 2, p + 64, 64, 0), "the source frames and the output overlap"),
        (u16, (p, 2, 128, 0, 8, 8, 8, 4, 4, 9, 0, 2, o, 128, 0), "depth 10 or 12 (8 bits: savsr_video_denoise_u8)"),
        (u16, (p + 1, 2, 128, 0, 8, 8, 10, 4, 4, 9, 0, 2, o, 128, 0), "2-byte aligned"),
        (u16, (p, 2, 130, 1, 8, 8, 10, 4, 4, 9, 0, 2, o, 128, 0), "2-byte aligned"),
        (u16, (p, 2, 128, 0, 8, 8, 10, 4, 4, 9, 0, 2, o + 1, 128, 0), "2-byte aligned"),
        (u16, (p, 2, 127, 0, 8, 8, 10, 4, 4, 9, 0, 2, o, 128, 0), "frame_bytes smaller"),
        (u16, (p, 2, 128, 0, 8, 8, 12, 33, 4, 9, 0, 2, o, 128, 0), "radius 1 .. 16"),
    ]
    for fn, args, words in bad:
        assert fn(*args, None) == -1, (fn.__name__, args)          # SAVSR_E_ARG
        msg = lib.savsr_last_error().decode()
        assert words in msg and fn.__name__[len("savsr_"):] in msg, (fn.__name__, args, msg)
    torch.cuda.synchronize()
    assert not out.any()                                             # refused before the device is touched: no launch left behind


# ---------------------------------------------------------------------------------------------------------------------- frames
def _planar(rng, n, h, w, depth, layout):
    planes = [walk_video(rng, n, *hw, depth) for hw in ([(h, w)] + ([] if layout == "400" else [yuv.chroma_hw(h, w, layout)] * 2))]
    frames = np.concatenate([as_bytes(p) for p in planes], 1)
    assert frames.shape[1] == yuv.frame_bytes(h, w, depth, layout)
    return np.ascontiguousarray(frames)


def test_denoise_video_of_every_frame_kind():
    rng = np.random.default_rng(30)
    for c in (1, 3):
        for h, w in ((5, 11), (8, 16)):          # frames of 55 / 165 bytes (one-sample form) and of 128 / 384 (vector form)
            v = walk_video(rng, 10, h, w * c).reshape(10, h, w, c)
            got = savsr_amd.denoise_video(torch.from_numpy(v))
            assert got.device.type == "cuda" and got.dtype == torch.uint8 and got.shape == v.shape
            assert np.array_equal(got.cpu().numpy(), denoise_frames(v)), (c, h, w)
            got = savsr_amd.denoise_video(torch.from_numpy(v).to(DEV), radius=2, strength=(3, 5))
            assert np.array_equal(got.cpu().numpy(), denoise_frames(v, radius=2, strength=(3, 5)))
    for fmt, layout, depth, (h, w) in (("i420", "420", 8, (7, 9)), ("i420", "420", 8, (16, 64)), ("i422", "422", 8, (8, 16)),
                                       ("i444", "444", 8, (6, 8)), ("y400", "400", 8, (5, 33)), ("i420", "420", 10, (16, 64)),
                                       ("i420", "420", 10, (7, 9)), ("i444", "444", 12, (4, 8))):
        frames = _planar(rng, 12, h, w, depth, layout)
        for cs in (None, (1, 2)):
            got = savsr_amd.denoise_video(torch.from_numpy(frames), fmt, (h, w), depth, 4, (4, 9), cs)
            want = denoise_frames(frames, fmt, (h, w), depth, 4, (4, 9), cs)
            assert np.array_equal(got.cpu().numpy(), want), (fmt, depth, h, w, cs)
        if layout != "400":          # the chroma strength reaches the chroma planes alone
            ysz = h * w * (2 if depth > 8 else 1)
            a = denoise_frames(frames, fmt, (h, w), depth, 4, (4, 9), None)
            b = denoise_frames(frames, fmt, (h, w), depth, 4, (4, 9), (0, 0))
            assert np.array_equal(a[:, :ysz], b[:, :ysz]) and np.array_equal(b[:, ysz:], frames[:, ysz:]) and not np.array_equal(a, b)
    one = torch.from_numpy(walk_video(rng, 1, 1, 3).reshape(1, 1, 1, 3))          # one frame of one row: nothing to average
    assert torch.equal(savsr_amd.denoise_video(one).cpu(), one)
    with pytest.raises(ValueError, match="float frames have no integer samples to denoise"):
        savsr_amd.denoise_video(torch.zeros(3, 3, 4, 4, device=DEV))


@pytest.mark.parametrize("chunk", [1, 2, 5, 14])
def test_temporal_denoiser_any_chunking(chunk):
    from savsr_amd.frames import detector_side
    from savsr_amd.prepass import TemporalDenoiser
    rng = np.random.default_rng(31)
    n = 14
    rgb = torch.from_numpy(walk_video(rng, n, 6, 16 * 3).reshape(n, 6, 16, 3)).to(DEV)
    yv = torch.from_numpy(_planar(rng, n, 7, 9, 10, "420")).to(DEV)
    for v, fmt, size, depth in ((rgb, "rgb", None, 8), (yv, "i420", (7, 9), 10)):
        for radius in (1, 4):
            whole = savsr_amd.denoise_video(v, fmt, size, depth, radius, (4, 9), (2, 4))
            stage = TemporalDenoiser(*detector_side(fmt, size, depth), radius, (4, 9), (2, 4))
            parts = []
            for a in range(0, n, chunk):
                parts.append(stage.push(v[a:a + chunk]))
                assert stage.held <= 2 * radius
            parts.append(stage.finish())
            assert torch.equal(torch.cat(parts, 0), whole), (fmt, radius, chunk)
            assert stage.held == 0 and stage.finish() is None


# ---------------------------------------------------------------------------------------------------------------------- the property
H = W = 16
N = 12


def _noisy(seed, n=N, h=H, w=W, c=3):
    return torch.from_numpy(walk_video(np.random.default_rng(seed), n, h, w * c).reshape(n, h, w, c))


def test_property_uint8_with_cuts_and_crop(net3):
    v = _noisy(40)
    clean = savsr_amd.denoise_video(v, radius=2, strength=(4, 9))
    assert not torch.equal(clean.cpu(), v)
    kw = dict(denoise="ata", denoise_radius=2)
    want = net3.upscale_video(clean, scale=2, out="uint8")
    got = net3.upscale_video(v, scale=2, out="uint8", **kw)
    assert got.shape == want.shape and torch.equal(got, want)
    assert not torch.equal(got, net3.upscale_video(v, scale=2, out="uint8"))
    assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", denoise=None), net3.upscale_video(v, scale=2, out="uint8"))
    # cuts="auto" scores the denoised frames
    assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", cuts="auto", scene_threshold=1.0, **kw),
                       net3.upscale_video(clean, scale=2, out="uint8", cuts="auto", scene_threshold=1.0))
    # the stage runs in front of the crop, and -- the rule being per sample -- commutes with it: cropping first by hand gives the same
    rect = (2, 4, 8, 12)
    got = net3.upscale_video(v, scale=2, out="uint8", crop=rect, bars="drop", **kw)
    assert torch.equal(got, net3.upscale_video(clean, scale=2, out="uint8", crop=rect, bars="drop"))
    by_hand = v[:, 2:10, 4:16].contiguous()
    assert torch.equal(savsr_amd.denoise_video(by_hand, radius=2), clean[:, 2:10, 4:16])
    assert torch.equal(got, net3.upscale_video(by_hand, scale=2, out="uint8", **kw))


def test_property_behind_fields_and_pulldown(net3):
    v = _noisy(41, n=10)
    kw = dict(denoise="ata", denoise_radius=2, denoise_strength=(5, 12))
    prog = savsr_amd.deinterlace(v, "tff")
    want = net3.upscale_video(savsr_amd.denoise_video(prog, radius=2, strength=(5, 12)), scale=2, out="uint8")
    got = net3.upscale_video(v, scale=2, out="uint8", fields="tff", **kw)
    assert got.shape[0] == 20 and torch.equal(got, want)
    film = savsr_amd.remove_pulldown(v, "tff")
    want = net3.upscale_video(savsr_amd.denoise_video(film, radius=2, strength=(5, 12)), scale=2, out="uint8")
    got = net3.upscale_video(v, scale=2, out="uint8", pulldown="tff", **kw)
    assert got.shape[0] == 8 and torch.equal(got, want)


def test_property_planar_and_surface(net3):
    frames = torch.from_numpy(_planar(np.random.default_rng(42), N, H, W, 8, "420"))
    fmt = dict(pixel_format="i420", size=(H, W), out="i420")
    kw = dict(denoise="ata", denoise_radius=3, denoise_chroma_strength=(2, 4))
    clean = savsr_amd.denoise_video(frames, "i420", (H, W), 8, 3, (4, 9), (2, 4))
    want = net3.upscale_video(clean, scale=2, **fmt)
    assert torch.equal(net3.upscale_video(frames, scale=2, **fmt, **kw), want)
    nv12 = savsr_amd.pack_surface(frames, Surface.nv12(pitch=32), "i420", (H, W))
    assert torch.equal(net3.upscale_video(nv12, scale=2, surface=Surface.nv12(pitch=32), **fmt, **kw), want)


def test_video_upscaler_in_chunks_of_five(net3):
    from savsr_amd import VideoUpscaler
    v = _noisy(43)
    for extra in ({}, dict(fields="tff"), dict(crop=(2, 4, 8, 12), cuts="auto", scene_threshold=1.0)):
        kw = dict(denoise="ata", denoise_radius=2, **extra)
        whole = net3.upscale_video(v, scale=2, out="uint8", **kw)
        up = VideoUpscaler(net3, 2, out="uint8", **kw)
        parts = []
        for a in range(0, N, 5):
            parts.append(up.push(v[a:a + 5]))
            assert up._noise.held <= 4
        parts.append(up.finish())
        assert torch.equal(torch.cat(parts, 0), whole), extra


def test_refused_arguments_leave_no_launch_behind(net3):
    from savsr_amd import VideoUpscaler
    v = _noisy(44)
    lib = _lib()
    assert lib.savsr_video_denoise_u8(0, 1, 1, 0, 1, 1, 1, 0, 0, 0, 1, 0, 1, 0, None) == -1          # a known last error to compare against
    before = lib.savsr_last_error()
    for call in (lambda **kw: net3.upscale_video(v, scale=2, out="uint8", **kw), lambda **kw: VideoUpscaler(net3, 2, out="uint8", **kw)):
        for kw, words in ((dict(denoise="nlmeans"), "denoise = 'nlmeans'"), (dict(denoise_radius=3), "goes with denoise="),
                          (dict(denoise="ata", denoise_radius=0), "denoise_radius = 0"),
                          (dict(denoise="ata", denoise_strength=(9, 4)), r"denoise_strength = \(9, 4\)")):
            with pytest.raises(ValueError, match=words):
                call(**kw)
    with pytest.raises(ValueError, match="float frames have no integer samples to denoise"):
        net3.upscale_video(torch.zeros(8, 3, H, W, device=DEV), scale=2, denoise="ata")
    assert lib.savsr_last_error() == before and b"video_denoise_u8: null pointer" in before
