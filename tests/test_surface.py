"""Video surfaces on the host: savsr_amd/surface.py, the numpy specification of unpack_surface / pack_surface (csrc/surface.hip), and the
refusals of the surface= / out_surface= arguments of upscale_video and VideoUpscaler.  No GPU."""
import numpy as np
import pytest
import torch

import savsr_amd
from savsr_amd import surface as S
from savsr_amd import yuv
from savsr_amd.surface import Surface
from tests import surface_cases as SC


# ------------------------------------------------------------------------------------------------------------------ the specification
@pytest.mark.parametrize("kind", S.KINDS)
def test_pack_then_unpack_is_the_identity(kind):
    for case in SC.BY_KIND[kind]:
        planar = SC.planar_frames(case)
        packed = S.pack_frames(planar, case.surface, case.h, case.w, case.depth, case.layout)
        assert packed.shape == (SC.N_FRAMES, case.table.bytes), case.id
        assert np.array_equal(S.unpack_frames(packed, case.surface, case.h, case.w, case.depth, case.layout), planar), case.id
        # a larger frame stride and random bits wherever no sample lies change nothing
        assert np.array_equal(S.unpack_frames(SC.surface_frames(case), case.surface, case.h, case.w, case.depth, case.layout), planar), case.id


def _words(a):
    return np.asarray(a, dtype="<u2").view(np.uint8).reshape(1, -1)


def test_unpack_equals_hand_built_frames_4x4():
    Y = np.arange(16).reshape(4, 4) + 100
    U, V = np.array([[1, 2], [3, 4]]), np.array([[11, 12], [13, 14]])
    planar = np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)]).astype(np.uint8)[None]
    nv12 = np.array([[100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 112, 113, 114, 115,
                      1, 11, 2, 12, 3, 13, 4, 14]], dtype=np.uint8)
    assert np.array_equal(S.unpack_frames(nv12, Surface.nv12(), 4, 4), planar)
    assert np.array_equal(S.pack_frames(planar, Surface.nv12(), 4, 4), nv12)
    nv21 = nv12.copy()
    nv21[0, 16:] = [11, 1, 12, 2, 13, 3, 14, 4]
    assert np.array_equal(S.unpack_frames(nv21, Surface.nv21(), 4, 4), planar)
    # P010: the same samples times 4 in 10 bits, in the high bits of the words
    p10 = _words([int(s) * 4 for s in planar[0]])
    p010 = _words([int(s) * 4 << 6 for s in nv12[0]])
    assert np.array_equal(S.unpack_frames(p010, Surface.p010(), 4, 4, 10), p10)
    assert np.array_equal(S.pack_frames(p10, Surface.p010(), 4, 4, 10), p010)
    # UYVY, 4:2:2: chroma planes of 4 x 2
    U2, V2 = np.arange(8).reshape(4, 2) + 1, np.arange(8).reshape(4, 2) + 11
    p422 = np.concatenate([Y.reshape(-1), U2.reshape(-1), V2.reshape(-1)]).astype(np.uint8)[None]
    uyvy = np.array([[1, 100, 11, 101, 2, 102, 12, 103,
                      3, 104, 13, 105, 4, 106, 14, 107,
                      5, 108, 15, 109, 6, 110, 16, 111,
                      7, 112, 17, 113, 8, 114, 18, 115]], dtype=np.uint8)
    assert np.array_equal(S.unpack_frames(uyvy, Surface.uyvy(), 4, 4, 8, "422"), p422)
    assert np.array_equal(S.pack_frames(p422, Surface.uyvy(), 4, 4, 8, "422"), uyvy)
    yuyv = uyvy.reshape(-1, 2)[:, ::-1].reshape(1, -1)
    assert np.array_equal(S.unpack_frames(yuyv, Surface.yuyv(), 4, 4, 8, "422"), p422)


def test_unpack_equals_hand_built_frames_3x5_with_pitch():
    """Odd sizes: chroma planes of 2 x 3 (4:2:0) / 3 x 3 (4:2:2); pitch 8 and 4 lines; X marks bytes that hold no sample."""
    X = 0xEE
    Y = np.arange(15).reshape(3, 5) + 100
    U, V = np.arange(6).reshape(2, 3) + 1, np.arange(6).reshape(2, 3) + 11
    planar = np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)]).astype(np.uint8)[None]
    nv12 = np.array([[100, 101, 102, 103, 104, X, X, X,
                      105, 106, 107, 108, 109, X, X, X,
                      110, 111, 112, 113, 114, X, X, X,
                      X, X, X, X, X, X, X, X,
                      1, 11, 2, 12, 3, 13, X, X,
                      4, 14, 5, 15, 6, 16, X, X]], dtype=np.uint8)
    s = Surface.nv12(pitch=8, lines=4)
    tab = s.resolve(3, 5)
    assert (tab.bytes, tab.planes[1].offset, tab.planes[1].rows, tab.planes[1].groups) == (48, 32, 2, 3)
    assert np.array_equal(S.unpack_frames(nv12, s, 3, 5), planar)
    assert np.array_equal(S.pack_frames(planar, s, 3, 5), np.where(nv12 == X, 0, nv12))
    p10 = _words([int(v) * 4 + 3 for v in planar[0]])
    p010 = _words([X if v == X else ((int(v) * 4 + 3) << 6) | 0x2A for v in nv12[0]])          # random low bits, pitch 16
    s = Surface.p010(pitch=16, lines=4)
    assert np.array_equal(S.unpack_frames(p010, s, 3, 5, 10), p10)
    U2, V2 = np.arange(9).reshape(3, 3) + 1, np.arange(9).reshape(3, 3) + 11
    p422 = np.concatenate([Y.reshape(-1), U2.reshape(-1), V2.reshape(-1)]).astype(np.uint8)[None]
    uyvy = np.array([[1, 100, 11, 101, 2, 102, 12, 103, 3, 104, 13, X,
                      4, 105, 14, 106, 5, 107, 15, 108, 6, 109, 16, X,
                      7, 110, 17, 111, 8, 112, 18, 113, 9, 114, 19, X]], dtype=np.uint8)
    assert np.array_equal(S.unpack_frames(uyvy, Surface.uyvy(), 3, 5, 8, "422"), p422)
    assert np.array_equal(S.pack_frames(p422, Surface.uyvy(), 3, 5, 8, "422"), np.where(uyvy == X, 0, uyvy))          # the pad Y is 0


def test_low_bits_of_msb_sources_are_ignored_and_high_samples_clamped():
    for kind in ("p010", "p012", "p210", "p212"):
        for case in SC.BY_KIND[kind]:
            a, b = SC.surface_frames(case), SC.surface_frames(case, 1)
            low = np.tile(_words([(1 << (16 - case.depth)) - 1]), case.stride // 2)[0]
            assert np.any((a ^ b) & low)                       # the low bits differ between the two
            args = (case.surface, case.h, case.w, case.depth, case.layout)
            assert np.array_equal(S.unpack_frames(a, *args), S.unpack_frames(b, *args)), case.id
    over = _words([0xFFFF] * 6)                                # samples above the depth's range are written as the largest one
    assert np.array_equal(S.pack_frames(over, Surface.p010(), 2, 2, 10), _words([0xFFC0] * 6))
    assert np.array_equal(S.pack_frames(over, Surface.planar(), 2, 2, 10), over)          # verbatim without msb


@pytest.mark.parametrize("kind", S.KINDS)
def test_uncovered_bytes_of_a_packed_surface_are_zero(kind):
    for case in SC.BY_KIND[kind]:
        mask = SC.sample_mask(case)
        assert not np.any(SC.packed_frames(case) & ~mask), case.id
        if case.pitch in ("aligned", "vector", "odd") or (case.kind in ("uyvy", "yuyv") and case.w % 2):
            assert np.any(mask == 0), case.id                  # there are such bytes
        if case.table.msb:
            assert np.all(mask.view("<u2")[mask.view("<u2") != 0] == (0xFFFF << (16 - case.depth)) & 0xFFFF), case.id


def test_resolve_gives_the_decoder_layout():
    tab = Surface.nv12(pitch_align=256, lines_align=16).resolve(1080, 1920)
    y, c = tab.planes
    assert (tab.bytes, tab.sample, tab.msb) == (2048 * 1088 * 3 // 2, 1, False)
    assert (y.offset, y.pitch, y.rows, y.groups, y.step) == (0, 2048, 1080, 1920, 1)
    assert (c.offset, c.pitch, c.rows, c.groups, c.step) == (2048 * 1088, 2048, 540, 960, 2)
    assert c.streams == (S.Stream(1, 1, 0), S.Stream(2, 1, 0)) and not tab.tight and tab.span == 2048 * 1088 + 539 * 2048 + 1920
    tab = Surface.p010(pitch_align=64).resolve(1080, 1920, 10)
    assert (tab.bytes, tab.sample, tab.msb, tab.planes[1].offset, tab.planes[1].pitch) == (3840 * 1620, 2, True, 3840 * 1080, 3840)
    tab = Surface.planar(pitch=2048, lines=1088).resolve(1080, 1920)
    assert [(p.offset, p.pitch, p.rows, p.groups) for p in tab.planes] == [(0, 2048, 1080, 1920), (2048 * 1088, 1024, 540, 960),
                                                                          (2048 * 1088 + 1024 * 544, 1024, 540, 960)]
    assert tab.bytes == 2048 * 1088 + 2 * 1024 * 544
    tab = Surface.planar(pitch=80, lines=8, chroma_pitch=48).resolve(6, 34, 10, "422")
    assert [(p.offset, p.pitch) for p in tab.planes] == [(0, 80), (640, 48), (1024, 48)] and tab.bytes == 1408
    tab = Surface.uyvy(pitch_align=64).resolve(480, 720, 8, "422")
    assert (tab.bytes, tab.planes[0].pitch, tab.planes[0].groups, tab.planes[0].step) == (1472 * 480, 1472, 360, 4)
    assert tab.planes[0].streams == (S.Stream(1, 1, 0), S.Stream(0, 2, 0), S.Stream(2, 1, 0), S.Stream(0, 2, 1))
    assert Surface.planar().resolve(5, 7, 8, "400").planes == (S.SurfacePlane(0, 7, 5, 7, (S.Stream(0, 1, 0),)),)
    for case in SC.CASES:                                          # the default is tight rows and no padding
        if case.pitch == "tight" and (case.kind == "planar" or case.w % 2 == 0):
            assert case.table.bytes == yuv.frame_bytes(case.h, case.w, case.depth, case.layout) and case.table.tight, case.id


@pytest.mark.parametrize("make,args,match", [
    (lambda: Surface.nv12(pitch=7), (4, 8), r"pitch = 7 below the 8 bytes of a row of plane 0"),
    (lambda: Surface.nv12(pitch=7), (4, 7), r"pitch = 7 below the 8 bytes of a row of plane 1 \(8 samples of 1 byte; a chroma row of odd width w has 2 \* ceil\(w / 2\) samples\)"),
    (lambda: Surface.nv16(pitch=9), (3, 9, 8, "422"), r"pitch = 9 below the 10 bytes of a row of plane 1"),
    (lambda: Surface.uyvy(pitch=18), (3, 9, 8, "422"), r"pitch = 18 below the 20 bytes of a row of plane 0"),
    (lambda: Surface.planar(pitch=8, chroma_pitch=3), (4, 8), r"chroma_pitch = 3 below the 4 bytes of a row of plane 1"),
    (lambda: Surface.nv12(lines=3), (4, 8), r"lines = 3 below the frame's 4 rows"),
    (lambda: Surface.p010(pitch=17), (4, 8, 10), r"pitch = 17 is odd: 10-bit samples are 16-bit words"),
    (lambda: Surface.planar(pitch=16, chroma_pitch=9), (4, 8, 12), r"chroma_pitch = 9 is odd: 12-bit samples are 16-bit words"),
    (lambda: Surface.p010(offsets=(0, 65)), (4, 8, 10), r"offset 65 of plane 1 is odd: 10-bit samples are 16-bit words"),
    (lambda: Surface.planar(msb=True), (4, 8), r"msb = True at depth 8"),
    (lambda: Surface.nv12(), (4, 8, 8, "422"), r"Surface.nv12\(\) holds I420 samples, the frames are I422"),
    (lambda: Surface.p010(), (4, 8, 8), r"Surface.p010\(\) holds 10-bit samples, the frames have depth = 8"),
    (lambda: Surface.p212(), (4, 8, 10, "422"), r"Surface.p212\(\) holds 12-bit samples, the frames have depth = 10"),
    (lambda: Surface.uyvy(), (4, 8), r"Surface.uyvy\(\) holds I422 samples, the frames are I420"),
    (lambda: Surface.uyvy(), (4, 8, 10, "422"), r"Surface.uyvy\(\) holds 8-bit samples, the frames have depth = 10"),
    (lambda: Surface.nv12(), (4, 8, 8, "400"), r"Surface.nv12\(\) holds I420 samples, the frames are Y400"),
    (lambda: Surface.nv12(offsets=(0, 31)), (4, 8), r"planes 0 and 1 overlap: bytes \[0, 32\) and \[31, 47\)"),
    (lambda: Surface.planar(offsets=(0, 32, 36)), (4, 8), r"planes 1 and 2 overlap: bytes \[32, 40\) and \[36, 44\)"),
    (lambda: Surface.nv12(offsets=(0,)), (4, 8), r"offsets = \(0,\): Surface.nv12\(\) of I420 frames has 2 planes"),
    (lambda: Surface.nv12(pitch=64, pitch_align=64), (4, 8), r"pitch_align = 64 together with pitch = 64"),
    (lambda: Surface.nv12(chroma_pitch=8), (4, 8), r"unexpected keyword argument 'chroma_pitch'"),
    (lambda: Surface("nv13"), (4, 8), r"surface kind = 'nv13': one of planar, nv12"),
    (lambda: Surface.nv12(pitch=0), (4, 8), r"pitch = 0: an int >= 1"),
])
def test_resolve_refuses_by_name(make, args, match):
    with pytest.raises((ValueError, TypeError), match=match):
        make().resolve(*args)


def test_frame_stride_of_surface_frames():
    s = Surface.nv12(pitch=16, lines=4)
    assert s.resolve(4, 8).bytes == 96
    with pytest.raises(ValueError, match="frame stride of 95 bytes, the surface takes 96"):
        S.unpack_frames(np.zeros((2, 95), np.uint8), s, 4, 8)
    assert S.unpack_frames(np.zeros((2, 101), np.uint8), s, 4, 8).shape == (2, 48)
    with pytest.raises(ValueError, match="odd frame stride of 195 bytes"):
        S.unpack_frames(np.zeros((2, 195), np.uint8), Surface.p010(pitch=32, lines=4), 4, 8, 10)
    with pytest.raises(ValueError, match="I420 frames of 4 x 8 have 48 bytes, got 47"):
        S.pack_frames(np.zeros((2, 47), np.uint8), s, 4, 8)
    with pytest.raises(TypeError, match="must be a savsr_amd.surface.Surface"):
        S.unpack_frames(np.zeros((2, 96), np.uint8), "nv12", 4, 8)


# ---------------------------------------------------------------------------------------------------- the public interface, on the host
def _net(**cfg):
    from savsr_amd.archs.savsr_arch import SAVSR
    return SAVSR(**cfg).eval()


def _frames(n, nbytes):
    return torch.zeros(n, nbytes, dtype=torch.uint8)


def test_pixel_format_nv12_is_still_an_unknown_format():
    with pytest.raises(ValueError, match="pixel_format = 'nv12': one of rgb, i420, i422, i444$"):
        _net().upscale_video(_frames(9, 120), pixel_format="nv12", size=(8, 10))
    with pytest.raises(ValueError, match="pixel_format = 'nv12': one of rgb, i420, i422, i444$"):
        _net().upscale_video(_frames(9, 120), pixel_format="nv12", size=(8, 10), surface=Surface.nv12())
    with pytest.raises(ValueError, match="pixel_format = 'nv12': one of rgb, i420, i422, i444$"):
        savsr_amd.unpack_surface(_frames(9, 120), Surface.nv12(), "nv12", (8, 10))
    with pytest.raises(ValueError, match="out = 'nv12': one of float, uint8, i420, i422, i444$"):
        _net().upscale_video(_frames(9, 120), pixel_format="i420", size=(8, 10), out="nv12")


I420 = dict(pixel_format="i420", size=(8, 10))


@pytest.mark.parametrize("kwargs,frames,exc,match", [
    (dict(surface=Surface.nv12()), torch.zeros(9, 8, 10, 3, dtype=torch.uint8), ValueError,
     r"surface = Surface.nv12\(\) goes with pixel_format = 'i420', 'i422', 'i444' or 'y400'.*'rgb' frames have none"),
    (dict(out="uint8", out_surface=Surface.nv12()), torch.zeros(9, 8, 10, 3, dtype=torch.uint8), ValueError,
     r"out_surface = Surface.nv12\(\) goes with out = 'i420', 'i422', 'i444' or 'y400'.*'uint8' frames have none"),
    (dict(out_surface=Surface.nv12(), **I420), _frames(9, 120), ValueError, r"out_surface = Surface.nv12\(\) goes with out = .*'float' frames have none"),
    (dict(surface="nv12", **I420), _frames(9, 120), TypeError, r"surface must be a savsr_amd.surface.Surface"),
    (dict(out="i420", out_surface="nv12", **I420), _frames(9, 120), TypeError, r"out_surface must be a savsr_amd.surface.Surface"),
    (dict(surface=Surface.nv12(pitch=16, lines=8), **I420), _frames(9, 120), ValueError, r"frame stride of 120 bytes, the surface takes 192"),
    (dict(surface=Surface.nv12(pitch=16, lines=8), **I420), _frames(9, 192)[0], ValueError, r"surface frames must be \[N, bytes\] uint8"),
    (dict(surface=Surface.nv12(pitch=16, lines=8), **I420), _frames(9, 192).float(), ValueError, r"surface frames must be \[N, bytes\] uint8"),
    (dict(surface=Surface.nv16(), **I420), _frames(9, 160), ValueError, r"Surface.nv16\(\) holds I422 samples, the frames are I420"),
    (dict(surface=Surface.p010(), **I420), _frames(9, 240), ValueError, r"Surface.p010\(\) holds 10-bit samples, the frames have depth = 8"),
    (dict(surface=Surface.uyvy(), **I420), _frames(9, 160), ValueError, r"Surface.uyvy\(\) holds I422 samples, the frames are I420"),
    (dict(surface=Surface.nv12(pitch=9), **I420), _frames(9, 120), ValueError, r"pitch = 9 below the 10 bytes of a row of plane 0"),
    (dict(out="i422", out_surface=Surface.nv12(), **I420), _frames(9, 120), ValueError, r"Surface.nv12\(\) holds I420 samples, the frames are I422"),
    (dict(out="i420", out_depth=10, out_surface=Surface.nv12(), **I420), _frames(9, 120), ValueError, r"Surface.nv12\(\) holds 8-bit samples, the frames have depth = 10"),
    (dict(out="i420", out_surface=Surface.nv12(pitch=39), scale=4, **I420), _frames(9, 120), ValueError, r"pitch = 39 below the 40 bytes of a row of plane 0"),
    (dict(out="i420", out_surface=Surface.nv12(pitch=16), scale=4, crop=(0, 2, 8, 4), bars="keep", **I420), _frames(9, 120), ValueError, r"pitch = 16 below the 40 bytes"),
    (dict(surface=Surface.nv12(), **I420), _frames(3, 120), ValueError, r"video has 3 frames: too few for a 7-frame 'reflection' window"),
    (dict(surface=Surface.nv12(pitch=16, lines=8), fields="tff", pixel_format="i420", size=(2, 10)), _frames(9, 192), ValueError, r"row"),
])
def test_upscale_video_refuses_bad_surface_arguments_without_a_gpu(kwargs, frames, exc, match):
    with pytest.raises(exc, match=match):
        _net().upscale_video(frames, **kwargs)


def test_valid_surface_arguments_reach_the_device_check():
    """Every host check passed: only the device is missing."""
    net = _net()
    for kw in (dict(surface=Surface.nv12(pitch=16, lines=8), out="i420", out_surface=Surface.nv12(pitch_align=64), **I420),
               dict(surface=Surface.nv12(pitch=16, lines=8), out="i420", out_surface=Surface.nv12(pitch=16), scale=4, crop=(0, 2, 8, 4), bars="drop", **I420),
               dict(surface=Surface.nv12(pitch=16, lines=8), fields="tff", crop="auto", out="i444", out_surface=Surface.planar(pitch_align=32), **I420)):
        with pytest.raises(RuntimeError, match="AMD GPU only"):
            net.upscale_video(_frames(9, 197), **kw)
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        net.upscale_video(_frames(9, 320), pixel_format="i422", size=(8, 10), depth=10, surface=Surface.p210(), out="i420",
                          out_depth=12, out_surface=Surface.p012(lines_align=16))
    with pytest.raises(ValueError, match="surface = Surface.nv12"):
        net.upscale_video(_frames(9, 197), surface=Surface.nv12())
    with pytest.raises(TypeError, match="positional"):          # keyword only, behind the existing parameters
        net.upscale_video(_frames(9, 120), None, "reflection", "float", "i420", (8, 10), None, 10.0, "bt601", None, 8, None, None, None, None, None, 24,
                          "keep", None, None, 5, Surface.nv12())


def test_video_upscaler_checks_surface_arguments_at_construction_and_push():
    from savsr_amd import VideoUpscaler
    net = _net()
    with pytest.raises(ValueError, match=r"surface = Surface.uyvy\(\) goes with pixel_format"):
        VideoUpscaler(net, surface=Surface.uyvy())
    with pytest.raises(ValueError, match=r"out_surface = Surface.nv12\(\) goes with out"):
        VideoUpscaler(net, out="uint8", out_surface=Surface.nv12())
    with pytest.raises(ValueError, match=r"Surface.uyvy\(\) holds I422 samples, the frames are I420"):
        VideoUpscaler(net, surface=Surface.uyvy(), **I420)
    with pytest.raises(ValueError, match=r"pitch = 16 below the 20 bytes"):
        VideoUpscaler(net, scale=2, out="i420", out_surface=Surface.nv12(pitch=16), **I420)
    up = VideoUpscaler(net, scale=2, out="i420", surface=Surface.nv12(pitch=16, lines=8), out_surface=Surface.nv12(pitch=32), **I420)
    with pytest.raises(ValueError, match="frame stride of 120 bytes, the surface takes 192"):
        up.push(_frames(4, 120))
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        up.push(_frames(4, 192))


def test_public_stage_calls_check_on_the_host():
    s = Surface.nv12(pitch=16, lines=8)
    with pytest.raises(ValueError, match=r"surface = Surface.nv12\(\) goes with pixel_format"):
        savsr_amd.unpack_surface(_frames(2, 192), s, "rgb")
    with pytest.raises(ValueError, match="frame stride of 191 bytes, the surface takes 192"):
        savsr_amd.unpack_surface(_frames(2, 191), s, "i420", (8, 10))
    with pytest.raises(ValueError, match=r"I420 frames of 8 x 10 are \[N, 120\] uint8"):
        savsr_amd.pack_surface(_frames(2, 121), s, "i420", (8, 10))
    with pytest.raises(ValueError, match=r"holds 8-bit samples, the frames have depth = 10"):
        savsr_amd.pack_surface(_frames(2, 240), s, "i420", (8, 10), 10)
    with pytest.raises(TypeError, match="must be a savsr_amd.surface.Surface"):
        savsr_amd.pack_surface(_frames(2, 120), None, "i420", (8, 10))
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        savsr_amd.unpack_surface(_frames(2, 192), s, "i420", (8, 10))
    assert savsr_amd.surface is S and savsr_amd.Surface is Surface
