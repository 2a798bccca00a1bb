"""GPU checks of the bwdif deinterlacer and the same-rate output: savsr_video_deinterlace_u8_m / _u16_m against the numpy
specification bit for bit (the shared inputs of tests/bwdif_cases.py, both forms of the kernels, both rates, ranges with context,
planes in place), method 0 against the entries without a method, the entries' refusals, FieldSplitter under any chunking, and the
property of upscale_video(fields=..., deinterlacer=..., field_rate=...): bit for bit the call on the deinterlaced video."""
import numpy as np
import pytest
import torch

import savsr_amd
from savsr_amd import yuv
from savsr_amd.deinterlace import FIELD_ORDERS, bwdif_matrix, deinterlace_frames, deinterlace_matrix
from savsr_amd.utils import synth
from tests.bwdif_cases import ORDERS, SHAPES, inputs
from tests.scan_cases import packed_case
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


def _run(mats, order, depth=8, method=1, rate=0, rng=None, off=0, before=0, after=0, step=1, old=False):
    """One `_m` entry (old=True: the entry without a method) on the matrices [N, R, C] as the plane `before` bytes into frames of before +
    plane + after bytes, the first frame `off` bytes past a 256-byte aligned allocation; source frames [rng) (default: all).  The output
    frames have the same layout, are poisoned first and are followed by guard bytes: nothing outside the planes is written.  Returns
    [2 n or n, R, C]."""
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
    no = (1 if rate else 2) * (hi - lo)
    dst = torch.full((no * fb + off + 64,), POISON, dtype=torch.uint8, device=DEV)
    assert dst.data_ptr() % 256 == 0
    lib, st = _lib(), torch.cuda.current_stream().cuda_stream
    oid = FIELD_ORDERS.index(order)
    head = (src.data_ptr() + off, n, fb, before, r, c, depth if depth > 8 else step, oid, lo, hi, dst.data_ptr() + off, fb, before)
    if old:
        assert method == 0 and rate == 0
        rc = (lib.savsr_video_deinterlace_u16 if depth > 8 else lib.savsr_video_deinterlace_u8)(*head, st)
    else:
        rc = (lib.savsr_video_deinterlace_u16_m if depth > 8 else lib.savsr_video_deinterlace_u8_m)(*head, method, rate, st)
    assert rc == 0, lib.savsr_last_error()
    got = dst.cpu().numpy()
    assert (got[:off] == POISON).all() and (got[off + no * fb:] == POISON).all()
    got = got[off:off + no * fb].reshape(no, fb)
    assert (got[:, :before] == POISON).all() and (got[:, before + plane.shape[1]:] == POISON).all()
    got = got[:, before:before + plane.shape[1]]
    return np.ascontiguousarray(got).view("<u2").reshape(no, r, c) if depth > 8 else got.reshape(no, r, c)


def _want(mats, order, depth, rate, rng=None):
    lo, hi = rng or (0, mats.shape[0])
    want = bwdif_matrix(mats, order, depth)[0][2 * lo:2 * hi]
    return want[0::2] if rate else want


def _is_vec(r, c, depth, off=0, before=0, after=0):
    """Whether the launch takes the vector form: plane pointers, frame strides and a row's bytes are multiples of 16."""
    row = c * (2 if depth > 8 else 1)
    return (off + before) % 16 == 0 and (before + r * row + after) % 16 == 0 and row % 16 == 0


# ---------------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("rate", [0, 1])
@pytest.mark.parametrize("order", ORDERS)
def test_bwdif_u8_equals_the_spec(order, rate):
    """Every shape x input of bwdif_cases, from an aligned pointer (the rows of 16, 32, 48 and 272 bytes take the vector form, the others
    the one-sample form) and one byte off (the one-sample form for all): both equal the specification, so they equal each other."""
    forms = set()
    for r, c in SHAPES:
        for name, v in inputs(r, c):
            v = v.astype(np.uint8)
            want = _want(v, order, 8, rate)
            for off in (0, 1):
                forms.add(_is_vec(r, c, 8, off))
                got = _run(v, order, 8, 1, rate, off=off)
                assert np.array_equal(got, want), (r, c, name, order, rate, off, np.argwhere(got != want)[:4])
    assert forms == {True, False}


@pytest.mark.parametrize("rate", [0, 1])
@pytest.mark.parametrize("depth", [10, 12])
def test_bwdif_u16_equals_the_spec(depth, rate):
    """16-bit samples with codes above 2^d - 1 among them (read as 2^d - 1, copied as they are); aligned (vector form where a row's
    2 c bytes are a multiple of 16) and two bytes off (one-sample form)."""
    top = (1 << depth) - 1
    forms = set()
    for r, c in SHAPES:
        for name, v in inputs(r, c, top):
            v = v.astype(np.uint16)
            v[:, ::2, ::5] = 60000
            for order in ORDERS:
                want = _want(v, order, depth, rate)
                for off in (0, 2):
                    forms.add(_is_vec(r, c, depth, off))
                    got = _run(v, order, depth, 1, rate, off=off)
                    assert np.array_equal(got, want), (r, c, name, order, depth, rate, off, np.argwhere(got != want)[:4])
    assert forms == {True, False}


@pytest.mark.parametrize("rate", [0, 1])
def test_bwdif_ranges_with_context(rate):
    """The first, the last and a middle frame of five (and a run of three), with prev / next taken among the resident frames; a range
    without its context is another video."""
    v = np.random.RandomState(21).randint(0, 256, size=(5, 13, 48)).astype(np.uint8)
    w = np.random.RandomState(22).randint(0, 4096, size=(5, 13, 24)).astype(np.uint16)
    for rng in ((0, 1), (4, 5), (2, 3), (1, 4), (0, 5)):
        for order in ORDERS:
            for off in (0, 1):
                assert np.array_equal(_run(v, order, 8, 1, rate, rng=rng, off=off), _want(v, order, 8, rate, rng)), (rng, order, off)
            for off in (0, 2):
                assert np.array_equal(_run(w, order, 12, 1, rate, rng=rng, off=off), _want(w, order, 12, rate, rng)), (rng, order, off)
    for n in (1, 2):
        assert np.array_equal(_run(v[:n], "tff", 8, 1, rate), _want(v[:n], "tff", 8, rate))
    assert not np.array_equal(_run(v[2:3], "tff", 8, 1, rate), _want(v, "tff", 8, rate, (2, 3)))


def test_bwdif_planes_inside_frames_in_both_forms():
    """A plane offset and a frame stride that keep the 16-byte alignment (vector form) and ones that break it (one-sample form): the same
    matrices give the same bytes, the specification's, and the bytes around the plane stay as they were."""
    v = np.random.RandomState(23).randint(0, 256, size=(3, 13, 48)).astype(np.uint8)
    w = np.random.RandomState(24).randint(0, 1024, size=(3, 10, 32)).astype(np.uint16)
    for mats, depth, places in ((v, 8, ((16, 32, True), (32, 0, True), (5, 3, False), (16, 8, False), (3, 13, False))),
                                (w, 10, ((16, 16, True), (6, 10, False), (2, 4, False)))):
        n, r, c = mats.shape
        for order in ORDERS:
            for rate in (0, 1):
                want = _want(mats, order, depth, rate)
                for before, after, vec in places:
                    assert _is_vec(r, c, depth, 0, before, after) == vec
                    got = _run(mats, order, depth, 1, rate, before=before, after=after)
                    assert np.array_equal(got, want), (depth, order, rate, before, after)


def test_method_0_is_the_entries_without_a_method():
    """Through the `_m` entries yadif gives the bytes of savsr_video_deinterlace_u8 / _u16 (and the specification's), and rate 1 their
    frames [0::2]; the pixel step still counts for it, and bwdif ignores it."""
    for r, c, step in ((9, 33, 1), (9, 33, 3), (10, 48, 3), (13, 48, 1), (33, 272, 4)):
        v = np.random.RandomState(r + c + step).randint(0, 256, size=(3, r, c)).astype(np.uint8)
        for order in ORDERS:
            old = _run(v, order, 8, 0, 0, step=step, old=True)
            assert np.array_equal(old, deinterlace_matrix(v, order, step)[0])
            assert np.array_equal(_run(v, order, 8, 0, 0, step=step), old)
            assert np.array_equal(_run(v, order, 8, 0, 1, step=step), old[0::2])
            assert np.array_equal(_run(v, order, 8, 0, 1, step=step, rng=(1, 3), off=1), old[2:6:2])
            assert np.array_equal(_run(v, order, 8, 1, 0, step=step), bwdif_matrix(v, order)[0])
    for r, c in ((9, 33), (10, 32)):
        w = np.random.RandomState(r).randint(0, 1024, size=(3, r, c)).astype(np.uint16)
        old = _run(w, "bff", 10, 0, 0, old=True)
        assert np.array_equal(old, deinterlace_matrix(w, "bff", 1, 10)[0])
        assert np.array_equal(_run(w, "bff", 10, 0, 0), old) and np.array_equal(_run(w, "bff", 10, 0, 1), old[0::2])


def test_new_entries_refuse_bad_arguments():
    lib = _lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    out = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p, o = buf.data_ptr(), out.data_ptr()
    u8, u16 = lib.savsr_video_deinterlace_u8_m, lib.savsr_video_deinterlace_u16_m
    # (frames, n_frames, frame_bytes, plane_offset, rows, row_bytes | cols, step | depth, order, from, to, out, out_frame_bytes, out_plane_offset, method, rate)
    bad = [
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 2, o, 64, 0, 2, 0), "method 0 (yadif) or 1 (bwdif)"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 2, o, 64, 0, -1, 0), "method 0 (yadif) or 1 (bwdif)"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 2, o, 64, 0, 1, 2), "rate 0 (double) or 1 (same)"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 2, o, 64, 0, 0, -1), "rate 0 (double) or 1 (same)"),
        (u16, (p, 2, 128, 0, 8, 8, 10, 0, 0, 2, o, 128, 0, 2, 0), "method 0 (yadif) or 1 (bwdif)"),
        (u16, (p, 2, 128, 0, 8, 8, 10, 0, 0, 2, o, 128, 0, 1, 3), "rate 0 (double) or 1 (same)"),
        # everything the entries without a method refuse
        (u8, (0, 2, 64, 0, 8, 8, 1, 0, 0, 2, o, 64, 0, 1, 0), "null pointer"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 2, 0, 64, 0, 1, 1), "null pointer"),
        (u8, (p, 0, 64, 0, 8, 8, 1, 0, 0, 0, o, 64, 0, 1, 0), "n_frames >= 1"),
        (u8, (p, 2, 64, 0, 1, 8, 1, 0, 0, 2, o, 64, 0, 1, 0), "rows >= 2"),
        (u8, (p, 2, 64, 0, 8, 0, 1, 0, 0, 2, o, 64, 0, 1, 0), "at least one sample"),
        (u8, (p, 2, 64, 0, 8, 8, 0, 0, 0, 2, o, 64, 0, 1, 0), "step 1 .. 4"),          # (ignored by bwdif, and still checked)
        (u8, (p, 2, 64, 0, 8, 8, 3, 0, 0, 2, o, 64, 0, 1, 0), "divisor of row_bytes"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 2, 0, 2, o, 64, 0, 1, 0), "order 0 (tff) or 1 (bff)"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, -1, 2, o, 64, 0, 1, 0), "0 <= from < to <= n_frames"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 3, o, 64, 0, 1, 1), "0 <= from < to <= n_frames"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 1, 1, o, 64, 0, 1, 1), "0 <= from < to <= n_frames"),
        (u8, (p, 2, 63, 0, 8, 8, 1, 0, 0, 2, o, 64, 0, 1, 0), "frame_bytes smaller"),
        (u8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 2, o, 64, 1, 1, 0), "out_frame_bytes smaller"),
        (u8, (p, 2, 64, -1, 8, 8, 1, 0, 0, 2, o, 64, 0, 1, 0), "plane offsets >= 0"),
        (u16, (p, 2, 128, 0, 8, 8, 8, 0, 0, 2, o, 128, 0, 1, 0), "depth 10 or 12"),
        (u16, (p + 1, 2, 128, 0, 8, 8, 10, 0, 0, 2, o, 128, 0, 1, 0), "2-byte aligned"),
        (u16, (p, 2, 130, 1, 8, 8, 10, 0, 0, 2, o, 128, 0, 1, 0), "2-byte aligned"),
        (u16, (p, 2, 127, 0, 8, 8, 10, 0, 0, 2, o, 128, 0, 1, 0), "frame_bytes smaller"),
        (u16, (p, 2, 128, 0, 1, 8, 10, 0, 0, 2, o, 128, 0, 1, 0), "rows >= 2"),
    ]
    for fn, args, words in bad:
        assert fn(*args, None) == -1, (fn.__name__, args)          # SAVSR_E_ARG
        msg = lib.savsr_last_error().decode()
        assert words in msg and fn.__name__[len("savsr_"):] in msg, (fn.__name__, args, msg)
    torch.cuda.synchronize()
    assert not out.any()                                                             # refused before the device is touched


# ---------------------------------------------------------------------------------------------------------------------- frames
@pytest.mark.parametrize("rate", ["double", "same"])
def test_public_deinterlace_with_bwdif_of_every_frame_kind(rate):
    rng = np.random.RandomState(30)
    for shape in ((3, 9, 11, 3), (3, 10, 16, 3)):          # rows of 33 bytes (one-sample form) and of 48 (vector form)
        rgb = rng.randint(0, 256, size=shape, dtype=np.uint8)
        for order in ORDERS:
            got = savsr_amd.deinterlace(torch.from_numpy(rgb), order, method="bwdif", rate=rate)
            assert got.device.type == "cuda" and got.dtype == torch.uint8 and got.shape[0] == (3 if rate == "same" else 6)
            assert np.array_equal(got.cpu().numpy(), deinterlace_frames(rgb, order, method="bwdif", rate=rate)), (shape, order)
    for fmt, layout, depth, (h, w) in (("i420", "420", 8, (10, 16)), ("i420", "420", 8, (9, 7)), ("i420", "420", 10, (10, 16)),
                                       ("i420", "420", 10, (9, 7)), ("y400", "400", 8, (9, 33))):
        fb = yuv.frame_bytes(h, w, depth, layout)
        frames = (rng.randint(0, 256, size=(3, fb), dtype=np.uint8) if depth == 8
                  else rng.randint(0, 1 << depth, size=(3, fb // 2)).astype("<u2").view(np.uint8).reshape(3, fb))
        got = savsr_amd.deinterlace(torch.from_numpy(frames).to(DEV), "tff", fmt, (h, w), depth, method="bwdif", rate=rate)
        assert np.array_equal(got.cpu().numpy(), deinterlace_frames(frames, "tff", fmt, (h, w), depth, "bwdif", rate)), (fmt, depth, h, w)
    # yadif at the same rate, and the defaults as they were
    rgb = rng.randint(0, 256, size=(3, 9, 16, 3), dtype=np.uint8)
    assert np.array_equal(savsr_amd.deinterlace(torch.from_numpy(rgb), "bff", rate=rate).cpu().numpy(), deinterlace_frames(rgb, "bff", rate=rate))
    assert np.array_equal(savsr_amd.deinterlace(torch.from_numpy(rgb), "bff").cpu().numpy(), deinterlace_frames(rgb, "bff"))
    with pytest.raises(ValueError, match="method = 'w3fdif'"):
        savsr_amd.deinterlace(torch.from_numpy(rgb), "tff", method="w3fdif")
    with pytest.raises(ValueError, match="rate = 'half'"):
        savsr_amd.deinterlace(torch.from_numpy(rgb), "tff", rate="half")


@pytest.mark.parametrize("chunk", [1, 2, 3])
@pytest.mark.parametrize("rate", ["double", "same"])
def test_field_splitter_with_bwdif_any_chunking(rate, chunk):
    from savsr_amd.frames import detector_side
    from savsr_amd.prepass import FieldSplitter
    v = torch.from_numpy(np.random.RandomState(31).randint(0, 256, size=(5, 10, 16, 3), dtype=np.uint8)).to(DEV)
    for method in ("bwdif", "yadif"):
        whole = savsr_amd.deinterlace(v, "tff", method=method, rate=rate)
        split = FieldSplitter("tff", *detector_side("rgb", None, 8), method, rate)
        parts = []
        for a in range(0, 5, chunk):
            parts.append(split.push(v[a:a + chunk]))
            assert split.held <= 2
        parts.append(split.finish())
        got = torch.cat(parts, 0)
        assert got.shape[0] == (5 if rate == "same" else 10) and torch.equal(got, whole), (method, rate, chunk)
        assert split.held == 0 and split.finish() is None


# ---------------------------------------------------------------------------------------------------------------------- the property
H = W = 16
N = 6


@pytest.mark.parametrize("rate,count", [("double", 12), ("same", 6)])
def test_property_uint8(net3, rate, count):
    v = np.random.RandomState(32).randint(0, 256, size=(N, H, W, 3), dtype=np.uint8)
    prog = savsr_amd.deinterlace(torch.from_numpy(v), "tff", method="bwdif", rate=rate)
    assert np.array_equal(prog.cpu().numpy(), deinterlace_frames(v, "tff", method="bwdif", rate=rate))
    want = net3.upscale_video(prog, scale=2, out="uint8")
    got = net3.upscale_video(torch.from_numpy(v), scale=2, out="uint8", fields="tff", deinterlacer="bwdif", field_rate=rate)
    assert got.shape[0] == count and got.shape == want.shape and torch.equal(got, want)
    # explicit cuts index the deinterlaced video: a cut at source frame 3 is 3 at the same rate and 6 at the double one
    k = 3 if rate == "same" else 6
    got = net3.upscale_video(torch.from_numpy(v), scale=2, out="uint8", fields="tff", deinterlacer="bwdif", field_rate=rate, cuts=[k])
    assert torch.equal(got, net3.upscale_video(prog, scale=2, out="uint8", cuts=[k]))
    with pytest.raises(ValueError, match=f"cut {count}"):
        net3.upscale_video(torch.from_numpy(v), scale=2, fields="tff", deinterlacer="bwdif", field_rate=rate, cuts=[count])


@pytest.mark.parametrize("rate,count", [("double", 12), ("same", 6)])
def test_property_i420(net3, rate, count):
    fb = yuv.frame_bytes(H, W, 8)
    v = np.random.RandomState(33).randint(0, 256, size=(N, fb), dtype=np.uint8)
    kw = dict(pixel_format="i420", size=(H, W))
    prog = savsr_amd.deinterlace(torch.from_numpy(v), "tff", "i420", (H, W), method="bwdif", rate=rate)
    want = net3.upscale_video(prog, scale=2, out="i420", **kw)
    got = net3.upscale_video(torch.from_numpy(v), scale=2, out="i420", fields="tff", deinterlacer="bwdif", field_rate=rate, **kw)
    assert got.shape[0] == count and torch.equal(got, want)


@pytest.mark.parametrize("rate,count", [("double", 12), ("same", 6)])
def test_video_upscaler_in_chunks_of_two(net3, rate, count):
    from savsr_amd import VideoUpscaler
    v = torch.from_numpy(np.random.RandomState(34).randint(0, 256, size=(N, H, W, 3), dtype=np.uint8))
    whole = net3.upscale_video(v, scale=2, out="uint8", fields="tff", deinterlacer="bwdif", field_rate=rate)
    up = VideoUpscaler(net3, 2, out="uint8", fields="tff", deinterlacer="bwdif", field_rate=rate)
    parts = []
    for a in range(0, N, 2):
        parts.append(up.push(v[a:a + 2]))
        assert up._split.held <= 2
    parts.append(up.finish())
    got = torch.cat(parts, 0)
    assert got.shape[0] == count and torch.equal(got, whole)


@pytest.mark.parametrize("rate,count", [("double", 16), ("same", 8)])
def test_scan_detect_takes_the_deinterlacer_and_the_rate(net3, rate, count):
    v = torch.from_numpy(packed_case("interlaced", "tff", 16, 20, motion=(2, 1), n=8))
    assert savsr_amd.detect_scan(v).kwargs() == {"fields": "tff"}
    want = net3.upscale_video(savsr_amd.deinterlace(v, "tff", method="bwdif", rate=rate), scale=2, out="uint8")
    got = net3.upscale_video(v, scale=2, out="uint8", scan="detect", deinterlacer="bwdif", field_rate=rate)
    assert got.shape[0] == count and torch.equal(got, want)
    assert torch.equal(got, net3.upscale_video(v, scale=2, out="uint8", fields="tff", deinterlacer="bwdif", field_rate=rate))


def test_the_new_keyword_arguments_are_refused_by_name(net3):
    from savsr_amd import VideoUpscaler
    v = torch.from_numpy(np.random.RandomState(35).randint(0, 256, size=(8, H, W, 3), dtype=np.uint8))
    for call in (lambda **kw: net3.upscale_video(v, scale=2, out="uint8", **kw), lambda **kw: VideoUpscaler(net3, 2, out="uint8", **kw)):
        with pytest.raises(ValueError, match=r"deinterlacer = 'bwdif' goes with fields="):
            call(deinterlacer="bwdif")
        with pytest.raises(ValueError, match=r"field_rate = 'same' goes with fields="):
            call(field_rate="same")
        with pytest.raises(ValueError, match=r"deinterlacer = 'bwdif' together with pulldown = 'tff'"):
            call(pulldown="tff", deinterlacer="bwdif")
        with pytest.raises(ValueError, match=r"field_rate = 'same' together with pulldown = 'bff'"):
            call(pulldown="bff", field_rate="same")
        with pytest.raises(ValueError, match=r"deinterlacer = 'w3fdif': one of yadif, bwdif"):
            call(fields="tff", deinterlacer="w3fdif")
        with pytest.raises(ValueError, match=r"field_rate = 'half': one of double, same"):
            call(fields="tff", field_rate="half")
        with pytest.raises(ValueError, match=r"deinterlacer = None: one of yadif, bwdif"):
            call(deinterlacer=None)
    with pytest.raises(TypeError):                                                   # keyword only
        net3.upscale_video(v, 2, "reflection", "uint8", "rgb", None, None, 10.0, "bt601", None, 8, None, None, None, None, None, 24, "keep", "tff",
                           None, 5, "bwdif")
    # the defaults, spelled out, are the call without them
    assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", fields="tff", deinterlacer="yadif", field_rate="double"),
                       net3.upscale_video(v, scale=2, out="uint8", fields="tff"))
    assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", deinterlacer="yadif", field_rate="double"),
                       net3.upscale_video(v, scale=2, out="uint8"))


# ---------------------------------------------------------------------------------------------------------------------- the CLI
def test_cli_deinterlacer_and_field_rate(net3, tmp_path):
    """--field-rate same: the Y4M output keeps the input's frame rate and is tagged Ip, a PNG folder holds N files."""
    import io
    import os

    from savsr_amd import io as sio
    from savsr_amd import y4m
    from savsr_amd.upscale import main
    n = 5
    frames = np.random.RandomState(36).randint(0, 256, size=(n, yuv.frame_bytes(H, W, 8)), dtype=np.uint8)
    f = io.BytesIO()
    y4m.Y4MWriter(f, W, H, (25, 1), "t", (1, 1)).write(frames)
    src, ckpt = tmp_path / "lr.y4m", tmp_path / "net.pth"
    src.write_bytes(f.getvalue())
    sio.save_network(net3, str(ckpt))
    kw = dict(out="i420", pixel_format="i420", size=(H, W))
    base = ["-i", str(src), "--scale", "2", "--checkpoint", str(ckpt), "--chunk", "2"]

    def expect(sr, fps):
        g = io.BytesIO()
        y4m.Y4MWriter(g, 2 * W, 2 * H, fps, "p", y4m.scaled_aspect((1, 1), (H, W), (2 * H, 2 * W))).write(sr.cpu().numpy())
        return g.getvalue()

    for rate, fps in (("same", (25, 1)), ("double", (50, 1))):
        dst = tmp_path / f"sr_{rate}.y4m"
        assert main(base + ["-o", str(dst), "--fields", "auto", "--deinterlacer", "bwdif", "--field-rate", rate]) == 0
        sr = net3.upscale_video(torch.from_numpy(frames), scale=2, fields="tff", deinterlacer="bwdif", field_rate=rate, **kw)
        assert sr.shape[0] == (n if rate == "same" else 2 * n)
        want = expect(sr, fps)
        assert dst.read_bytes() == want and f" F{fps[0]}:1 Ip ".encode() in want[:80]
    out_dir = tmp_path / "png"
    assert main(base + ["-o", str(out_dir), "--fields", "tff", "--field-rate", "same"]) == 0
    assert sorted(os.listdir(out_dir)) == [f"{k:08d}.png" for k in range(n)]
