"""GPU checks of the scan detection: savsr_video_field_stats_u8 / _u16 (csrc/scan.hip) against the numpy specification bit for bit (odd
sizes, the 16-byte form and the one-sample form, one scored row, no scored row, a row wider than a workgroup, every depth, an
unaligned pointer, clamped neighbours), ranges and the streaming accumulator, detect_scan against the specification's decision,
upscale_video(scan="detect") against the explicit call, the refusals, the CLI."""
import io
import json
import os

import numpy as np
import pytest
import torch

import savsr_amd
from savsr_amd import scan as sc
from savsr_amd import y4m, yuv
from savsr_amd.surface import Surface
from savsr_amd.utils import synth
from tests.scan_cases import expected, packed_case, planar_case
from tests.video_cases import WEIGHT_SEED

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N = 5


def _lib():
    from savsr_amd import _lib as L
    return L.load()


@pytest.fixture(scope="module")
def net3():
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=WEIGHT_SEED), strict=True)
    return net.to(DEV).eval()


def _packed(n, h, w, c, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=(n, h, w, c), dtype=np.uint8)


def _planar(n, h, w, depth, layout, seed=0):
    rng = np.random.RandomState(seed)
    fb = yuv.frame_bytes(h, w, depth, layout)
    if depth == 8:
        return rng.randint(0, 256, size=(n, fb), dtype=np.uint8)
    words = rng.randint(0, 1 << depth, size=(n, fb // 2))
    words[:, ::7] = 50000                                                            # above 2^d - 1: read as 2^d - 1
    return words.astype("<u2").view(np.uint8).reshape(n, fb)


def _same(got: torch.Tensor, want: np.ndarray, what):
    assert got.device.type == "cuda" and got.dtype == torch.int64 and tuple(got.shape) == want.shape, what
    assert np.array_equal(got.cpu().numpy(), want), (what, got.cpu().numpy().tolist(), want.tolist())


# ---------------------------------------------------------------------------------------------------------------------- kernel = spec
@pytest.mark.parametrize("shape", [(9, 17, 1), (7, 5, 3), (12, 16, 3), (3, 16, 1), (2, 16, 1), (5, 4112, 1)])
def test_field_stats_of_packed_frames_equal_the_spec(shape):
    """[N, 9, 17, 1] and [N, 7, 5, 3]: the one-sample form, odd everything; [N, 12, 16, 3]: the vector form, 48-byte rows; [N, 3, 16, 1]:
    one scored row, one parity only; [N, 2, 16, 1]: no comb rows, rep only; [N, 5, 4112, 1]: a row wider than a workgroup."""
    h, w, c = shape
    v = _packed(N, h, w, c, seed=h + w)
    want = sc.frame_stats(v)
    _same(savsr_amd.field_stats(torch.from_numpy(v)), want, shape)
    _same(savsr_amd.field_stats(torch.from_numpy(v).to(DEV)), want, shape)
    if h == 3:
        assert want[:, [0, 2, 4]].sum() == 0 and want[:, [1, 3, 5]].sum() > 0        # y = 1 alone lies between two rows
    if h == 2:
        assert not want[:, :6].any() and want[1:, 6:].all() and not want[0, 6:].any()


@pytest.mark.parametrize("case", [("i420", "420", 6, 10, 8), ("i420", "420", 10, 24, 10), ("i444", "444", 9, 7, 12), ("y400", "400", 8, 32, 8)])
def test_field_stats_of_planar_frames_equal_the_spec(case):
    """i420 6 x 10 at 8 bits (one-sample form), i420 10 x 24 at 10 bits (the u16 vector form), i444 9 x 7 at 12 bits (the u16 one-sample
    form), y400 8 x 32 (the vector form): the Y plane, samples above the depth clamped."""
    fmt, layout, h, w, depth = case
    frames = _planar(N, h, w, depth, layout, seed=h)
    want = sc.frame_stats(frames, fmt, (h, w), depth)
    _same(savsr_amd.field_stats(torch.from_numpy(frames), fmt, (h, w), depth), want, case)


def test_field_stats_from_a_pointer_one_byte_off():
    """A frames tensor that is a view at a 1-byte offset of its storage: a vector-sized shape through the one-sample form."""
    v = _packed(N, 12, 16, 3, seed=3)
    raw = torch.empty(v.size + 1, dtype=torch.uint8, device=DEV)
    view = raw[1:].view(N, 12, 16, 3)
    view.copy_(torch.from_numpy(v))
    assert view.data_ptr() % 16 == 1 and view.is_contiguous()
    _same(savsr_amd.field_stats(view), sc.frame_stats(v), "offset 1")


@pytest.mark.parametrize("n", [1, 2])
def test_field_stats_of_one_and_two_frames_clamp_the_neighbours(n):
    for shape in ((9, 17, 1), (12, 16, 3)):
        v = _packed(n, *shape, seed=n)
        want = sc.frame_stats(v)
        _same(savsr_amd.field_stats(torch.from_numpy(v)), want, (n, shape))
        assert not want[0, 6:].any() and np.array_equal(want[0, 0:2], want[0, 4:6])  # frame 0 is its own predecessor
        if n == 1:
            assert np.array_equal(want[0, 2:4], want[0, 4:6])


def test_field_stats_of_the_largest_lane_sums():
    """0 / 255 alternating by row parity and by frame: every sample adds the most it can; the 32-bit partials do not overflow."""
    tall = np.zeros((3, 2048, 64, 1), np.uint8)
    tall[:, 1::2] = 255
    tall[1] = 255 - tall[1]
    want = sc.frame_stats(tall)
    assert want[1, 0] == 0 and want[1, 4] == 1023 * 64 * 510 and want[1, 6] == 1024 * 64 * 255
    _same(savsr_amd.field_stats(torch.from_numpy(tall)), want, "tall")


def test_entries_refuse_bad_arguments():
    lib = _lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    out = torch.full((4096,), 0xA5, dtype=torch.uint8, device=DEV)
    p, o = buf.data_ptr(), out.data_ptr()
    s8, s16 = lib.savsr_video_field_stats_u8, lib.savsr_video_field_stats_u16
    bad = [
        # (frames, n_frames, frame_bytes, plane_offset, rows, row_bytes, lo, hi, out)
        (s8, (0, 2, 64, 0, 8, 8, 0, 2, o), "null pointer"),
        (s8, (p, 2, 64, 0, 8, 8, 0, 2, 0), "null pointer"),
        (s8, (p, 0, 64, 0, 8, 8, 0, 0, o), "n_frames >= 1"),
        (s8, (p, 2, 64, 0, 0, 8, 0, 2, o), "rows >= 1"),
        (s8, (p, 2, 64, 0, 8, 0, 0, 2, o), "at least one sample"),
        (s8, (p, 2, 64, 0, 8, 8, -1, 2, o), "0 <= lo <= hi <= n_frames"),
        (s8, (p, 2, 64, 0, 8, 8, 0, 3, o), "0 <= lo <= hi <= n_frames"),
        (s8, (p, 2, 64, 0, 8, 8, 2, 1, o), "0 <= lo <= hi <= n_frames"),
        (s8, (p, 2, 63, 0, 8, 8, 0, 2, o), "frame_bytes smaller"),
        (s8, (p, 2, 64, 1, 8, 8, 0, 2, o), "frame_bytes smaller"),
        (s8, (p, 2, 64, -1, 8, 8, 0, 2, o), "plane offsets >= 0"),
        (s8, (p, 2, 64, 0, 8, 8, 0, 2, o + 4), "8-byte aligned"),
        # (frames, n_frames, frame_bytes, plane_offset, rows, cols, depth, lo, hi, out)
        (s16, (p, 2, 128, 0, 8, 8, 8, 0, 2, o), "depth 10 or 12"),
        (s16, (p + 1, 2, 128, 0, 8, 8, 10, 0, 2, o), "2-byte aligned"),
        (s16, (p, 2, 129, 0, 8, 8, 10, 0, 2, o), "2-byte aligned"),
        (s16, (p, 2, 127, 0, 8, 8, 10, 0, 2, o), "frame_bytes smaller"),
        (s16, (p, 2, 128, 0, 8, 8, 12, 0, 2, 0), "null pointer"),
    ]
    torch.cuda.synchronize()
    for fn, args, words in bad:
        assert fn(*args, None) == -1, (fn.__name__, args)
        msg = lib.savsr_last_error().decode()
        assert words in msg and fn.__name__[len("savsr_"):] in msg, (fn.__name__, args, msg)
    assert s8(p, 2, 64, 0, 8, 8, 1, 1, o, None) == 0                                 # an empty range: nothing is done
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())                                                 # refused before the device is touched (not even the memset)


# ---------------------------------------------------------------------------------------------------------------------- ranges, chunking
def test_ranges_equal_the_rows_of_the_whole():
    from savsr_amd.frames import detector_side
    from savsr_amd.prepass import _field_stats_device
    v = _packed(N, 9, 16, 3, seed=5)
    want = sc.frame_stats(v)
    dev = torch.from_numpy(v).to(DEV)
    side, size = detector_side("rgb", None, 8)
    for lo, hi in ((0, 1), (1, 2), (1, 4), (4, 5), (0, 5), (2, 2)):
        _same(_field_stats_device(dev, side, size, lo, hi), want[lo:hi], (lo, hi))
    frames = _planar(N, 10, 24, 10, "420", seed=6)
    side, size = detector_side("i420", (10, 24), 10)
    want = sc.frame_stats(frames, "i420", (10, 24), 10)
    for lo, hi in ((1, 3), (3, 5)):
        _same(_field_stats_device(torch.from_numpy(frames).to(DEV), side, size, lo, hi), want[lo:hi], (lo, hi))
    # the range without its context is another video: frame 1 alone is its own neighbours
    assert not np.array_equal(savsr_amd.field_stats(dev[1:2]).cpu().numpy(), want[1:2])


@pytest.mark.parametrize("chunks", [(1,) * 6, (2, 3, 1), (6,)])
def test_scan_stats_of_any_chunking_equal_field_stats(chunks):
    from savsr_amd.frames import detector_side
    for fmt, size, depth, frames in (("rgb", None, 8, _packed(6, 9, 17, 3, seed=7)), ("i420", (10, 24), 10, _planar(6, 10, 24, 10, "420", seed=8))):
        whole = savsr_amd.field_stats(torch.from_numpy(frames), fmt, size, depth)
        acc = savsr_amd.ScanStats(*detector_side(fmt, size, depth))
        dev, parts, a = torch.from_numpy(frames).to(DEV), [], 0
        for k in chunks:
            parts.append(acc.push(dev[a:a + k]))
            a += k
            assert acc.held <= max(2, k)
            assert acc._src.untyped_storage().nbytes() <= max(2, k) * frames[0].size  # copies of their own: the chunk's storage is released
        parts.append(acc.finish())
        assert torch.equal(torch.cat(parts, 0), whole) and acc.held == 0 and acc.finish() is None


# ---------------------------------------------------------------------------------------------------------------------- the decision
KINDS = [("interlaced", "tff"), ("interlaced", "bff"), ("telecine", "tff"), ("telecine", "bff"), ("progressive", None), ("static", None)]


@pytest.mark.parametrize("size", [(12, 20), (36, 48)])
def test_detect_scan_equals_the_specification(size):
    h, w = size
    for kind, order in KINDS:
        for motion in ((1, 0), (2, 1)):
            v = packed_case(kind, order, h, w, motion=motion, noise=2)
            want = sc.verdict_from_stats(sc.frame_stats(v))
            got = savsr_amd.detect_scan(torch.from_numpy(v))
            assert got == want and isinstance(got, savsr_amd.ScanVerdict) and (got.scan, got.order) in expected(kind, order), (kind, order, motion)
            y = planar_case(kind, order, h, w, motion=motion)
            want = sc.verdict_from_stats(sc.frame_stats(y, "i420", (h, w)))
            got = savsr_amd.detect_scan(torch.from_numpy(y).to(DEV), "i420", (h, w))
            assert got == want and (got.scan, got.order) in expected(kind, order), (kind, order, motion)
    v = packed_case("interlaced", "tff", h, w, motion=(2, 1))
    got = savsr_amd.detect_scan(torch.from_numpy(v), interlace_threshold=1000)
    assert got == sc.verdict_from_stats(sc.frame_stats(v), interlace_threshold=1000) and got.scan == "undetermined"
    assert savsr_amd.detect_scan(torch.from_numpy(v[:2])).scan == "undetermined"


# ---------------------------------------------------------------------------------------------------------------------- the network
H, W = 16, 20


def _video(kind, order, n=8):
    return packed_case(kind, order, H, W, motion=(2, 1), n=n)


@pytest.mark.parametrize("kind,order", [("interlaced", "tff"), ("interlaced", "bff"), ("telecine", "bff"), ("progressive", None), ("static", None)])
def test_upscale_video_with_scan_detect_is_the_explicit_call(net3, kind, order):
    v = torch.from_numpy(_video(kind, order))
    verdict = savsr_amd.detect_scan(v)
    assert (verdict.scan, verdict.order) in expected(kind, order)
    assert verdict.kwargs() == ({"fields": order} if kind == "interlaced" else {"pulldown": order} if kind == "telecine" else {})
    want = net3.upscale_video(v, scale=2, out="uint8", **verdict.kwargs())
    got = net3.upscale_video(v, scale=2, out="uint8", scan="detect")
    n = v.shape[0]
    assert got.shape[0] == {"interlaced": 2 * n, "telecine": n - n // 5}.get(kind, n)
    assert got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(net3.upscale_video(v.to(DEV), scale=2, out="uint8", scan="detect"), want)


def test_scan_none_is_the_call_without_the_argument(net3):
    v = torch.from_numpy(_video("interlaced", "tff"))
    assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", scan=None), net3.upscale_video(v, scale=2, out="uint8"))


def test_scan_detect_with_cuts_crop_and_a_surface(net3):
    v = torch.from_numpy(_video("interlaced", "bff"))
    for more in (dict(cuts="auto"), dict(crop=(2, 4, 12, 12)), dict(cuts=[9])):       # (cut 9 exists among the 16 progressive frames only)
        want = net3.upscale_video(v, scale=2, out="uint8", fields="bff", **more)
        assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", scan="detect", **more), want), more
    with pytest.raises(ValueError, match="cut 9"):                                   # a progressive verdict: the 8 frames as they are
        net3.upscale_video(torch.from_numpy(_video("progressive", None)), scale=2, scan="detect", cuts=[9])
    with pytest.raises(ValueError, match="too few"):                                 # the length check sees the verdict's count: 2 frames, no fields
        net3.upscale_video(v[:2], scale=2, scan="detect")
    from savsr_amd import surface as S
    planar = planar_case("telecine", "tff", H, W, motion=(2, 1))
    surf = Surface.nv12(pitch=32, lines=16)
    frames = torch.from_numpy(S.pack_frames(planar, surf, H, W, 8, "420"))
    kw = dict(scale=2, pixel_format="i420", size=(H, W), out="i420")
    assert savsr_amd.detect_scan(torch.from_numpy(planar), "i420", (H, W)).kwargs() == {"pulldown": "tff"}
    want = net3.upscale_video(frames, surface=surf, pulldown="tff", **kw)
    assert want.shape[0] == 13 - 13 // 5
    assert torch.equal(net3.upscale_video(frames, surface=surf, scan="detect", **kw), want)
    assert torch.equal(net3.upscale_video(frames.to(DEV), surface=surf, scan="detect", out_surface=Surface.nv12(pitch=64), **kw),
                       net3.upscale_video(frames, surface=surf, pulldown="tff", out_surface=Surface.nv12(pitch=64), **kw))


def test_scan_refusals(net3):
    from savsr_amd import VideoUpscaler
    v = torch.from_numpy(_video("interlaced", "tff"))
    with pytest.raises(ValueError, match="scan = 'detect' together with fields = 'tff'"):
        net3.upscale_video(v, scale=2, scan="detect", fields="tff")
    with pytest.raises(ValueError, match="scan = 'detect' together with pulldown = 'tff'"):
        net3.upscale_video(v, scale=2, scan="detect", pulldown="tff")
    with pytest.raises(ValueError, match="scan = 'detect' with pulldown_cycle = 4"):
        net3.upscale_video(v, scale=2, scan="detect", pulldown_cycle=4)
    with pytest.raises(ValueError, match="scan = 'auto': None or 'detect'"):
        net3.upscale_video(v, scale=2, scan="auto")
    with pytest.raises(ValueError, match="float frames have no integer samples"):
        net3.upscale_video(v.to(DEV).float().permute(0, 3, 1, 2).contiguous() / 255, scale=2, scan="detect")
    with pytest.raises(ValueError, match="scan = 'detect' in VideoUpscaler.*detect_scan"):
        VideoUpscaler(net3, 2, scan="detect")
    with pytest.raises(ValueError, match="fields = 'auto'"):
        net3.upscale_video(v, scale=2, fields="auto")


# ---------------------------------------------------------------------------------------------------------------------- the CLI
def _y4m_bytes(sr, w, h, fps, tag, lr):
    g = io.BytesIO()
    y4m.Y4MWriter(g, w, h, fps, tag, y4m.scaled_aspect((1, 1), lr, (h, w))).write(sr.cpu().numpy())
    return g.getvalue()


def test_cli_scan_detect_on_a_y4m_file_with_a_wrong_tag(net3, tmp_path, capsys):
    """A file tagged Ip whose content is interlaced, top field first: --scan detect runs as --fields tff does."""
    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    frames = planar_case("interlaced", "tff", H, W, motion=(2, 1), n=8)
    f = io.BytesIO()
    y4m.Y4MWriter(f, W, H, (25, 1), "p", (1, 1)).write(frames)
    src, ckpt = tmp_path / "lr.y4m", tmp_path / "net.pth"
    src.write_bytes(f.getvalue())
    sio.save_network(net3, str(ckpt))
    base = ["-i", str(src), "--scale", "2", "--checkpoint", str(ckpt), "--chunk", "3"]
    got, explicit, verdict = tmp_path / "scan.y4m", tmp_path / "fields.y4m", tmp_path / "scan.json"
    assert main(base + ["-o", str(got), "--scan", "detect", "--scan-out", str(verdict)]) == 0
    cap = capsys.readouterr()
    assert "--scan detect: interlaced, top field first: --fields tff" in cap.err
    assert "tagged Ip, its content is interlaced, top field first" in cap.err and "scan interlaced, top field first" in cap.out
    assert main(base + ["-o", str(explicit), "--fields", "tff"]) == 0
    sr = net3.upscale_video(torch.from_numpy(frames), scale=2, fields="tff", out="i420", pixel_format="i420", size=(H, W))
    want = _y4m_bytes(sr, 2 * W, 2 * H, (50, 1), "p", (H, W))
    assert sr.shape[0] == 16 and b" F50:1 Ip " in want[:80]
    assert got.read_bytes() == explicit.read_bytes() == want
    j = json.loads(verdict.read_text())
    want_v = sc.detect_scan_frames(frames, "i420", (H, W))
    assert j == json.loads(json.dumps(want_v.as_json())) and j["scan"] == "interlaced" and j["order"] == "tff" and len(j["rep_field"]) == 8
    # --crop auto's first pass sees the deinterlaced frames the second pass will crop
    both, both_explicit = tmp_path / "scan_crop.y4m", tmp_path / "fields_crop.y4m"
    assert main(base + ["-o", str(both), "--scan", "detect", "--crop", "auto"]) == 0
    assert main(base + ["-o", str(both_explicit), "--fields", "tff", "--crop", "auto"]) == 0
    assert both.read_bytes() == both_explicit.read_bytes()
    with pytest.raises(SystemExit):
        main(["-i", "-", "-o", str(tmp_path / "x.y4m"), "--scale", "2", "--checkpoint", str(ckpt), "--scan", "detect"])
    assert "stdin does not allow" in capsys.readouterr().err


def test_cli_scan_detect_on_a_png_folder_of_telecined_frames(net3, tmp_path, capsys):
    from PIL import Image

    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    frames = packed_case("telecine", "bff", H, W, motion=(2, 1))
    src, ckpt = tmp_path / "lr", tmp_path / "net.pth"
    src.mkdir()
    for k, fr in enumerate(frames):
        Image.fromarray(fr).save(src / f"{k:04d}.png")
    sio.save_network(net3, str(ckpt))
    base = ["-i", str(src), "--scale", "2", "--checkpoint", str(ckpt), "--chunk", "4", "--fps", "30000:1001"]
    got, explicit = tmp_path / "scan.y4m", tmp_path / "pulldown.y4m"
    assert main(base + ["-o", str(got), "--scan", "detect"]) == 0
    cap = capsys.readouterr()
    assert "--scan detect: telecine, bottom field first: --pulldown bff" in cap.err and "tagged" not in cap.err
    assert main(base + ["-o", str(explicit), "--pulldown", "bff"]) == 0
    sr = net3.upscale_video(torch.from_numpy(frames), scale=2, pulldown="bff", out="i420")
    assert sr.shape[0] == 11 and got.read_bytes() == explicit.read_bytes() and b" F24000:1001 Ip " in got.read_bytes()[:80]
    with open(got, "rb") as f:
        r = y4m.Y4MReader(f)
        assert (r.fps, r.interlace, r.width, r.height) == ((24000, 1001), "p", 2 * W, 2 * H)
        assert np.array_equal(np.concatenate(list(r.chunks(4))), sr.cpu().numpy())
    out_dir = tmp_path / "png"
    assert main(base[:-2] + ["-o", str(out_dir), "--scan", "detect"]) == 0
    assert sorted(os.listdir(out_dir)) == [f"{k:08d}.png" for k in range(11)]
