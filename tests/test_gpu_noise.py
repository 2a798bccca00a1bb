"""GPU checks of the noise estimator: savsr_video_noise_stats_u8 / _u16 against the numpy specification bit for bit
(savsr_amd/noise.py), at the smallest shapes at which the kernels can go wrong (tests/noise_cases.py), the entries' refusals, the
Python surface, and the properties of upscale_video(denoise_strength="auto", spatial_strength="auto") and of the CLI's passes."""
import numpy as np
import pytest
import torch

import savsr_amd
from savsr_amd import noise as NZ
from savsr_amd.utils import synth
from tests.deblock_cases import as_bytes
from tests.noise_cases import SMALLEST, case_seed, checkerboard, flat_beside_binned, picture, stats_frames, stats_tile
from tests.video_cases import WEIGHT_SEED

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 8          # int64 cells on either side of a table


def _lib():
    from savsr_amd import _lib as L
    return L.load()


@pytest.fixture(scope="module")
def net3():
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=WEIGHT_SEED), strict=True)
    return net.to(DEV).eval()


def _place(m, off, before, after):
    """The samples [N, R, C, step] as the plane `before` bytes into frames of before + plane + after bytes, the first frame `off` bytes
    past a 256-byte aligned allocation that ends with the last frame: (the device buffer, frame bytes)."""
    n = m.shape[0]
    plane = as_bytes(m)
    fb = before + plane.shape[1] + after
    host = np.full((n, fb), 0x3C, np.uint8)
    host[:, before:before + plane.shape[1]] = plane
    src = torch.empty(n * fb + off, dtype=torch.uint8, device=DEV)
    assert src.data_ptr() % 256 == 0
    src[off:].copy_(torch.from_numpy(host).reshape(-1))
    return src, fb


def _stats(m, depth=8, interlaced=False, off=0, before=0, after=0, calls=1):
    """savsr_video_noise_stats_* `calls` times on one zeroed table between guard cells: int64 [N, 256, 2]."""
    n, r, c, step = m.shape
    src, fb = _place(m, off, before, after)
    out = torch.full((n * 512 + 2 * GUARD,), -7, dtype=torch.int64, device=DEV)
    out[GUARD:GUARD + n * 512] = 0
    lib, st = _lib(), torch.cuda.current_stream().cuda_stream
    head = (src.data_ptr() + off, n, fb, before, r, c, step) + ((depth,) if depth > 8 else ())
    fn = lib.savsr_video_noise_stats_u16 if depth > 8 else lib.savsr_video_noise_stats_u8
    for _ in range(calls):
        assert fn(*head, int(interlaced), out.data_ptr() + 8 * GUARD, st) == 0, lib.savsr_last_error()
    got = out.cpu().numpy()
    assert (got[:GUARD] == -7).all() and (got[GUARD + n * 512:] == -7).all()
    return got[GUARD:GUARD + n * 512].reshape(n, 256, 2)


def _check_stats(m, depth=8, interlaced=False, calls=1, **place):
    got = _stats(m, depth, interlaced, calls=calls, **place)
    want = np.stack([sum(NZ.noise_stats_matrix(m[t, :, :, ch], depth, interlaced) for ch in range(m.shape[3])) for t in range(m.shape[0])]) * calls
    assert np.array_equal(got, want), (m.shape, depth, interlaced, place, np.argwhere(got != want)[:4].tolist())
    return got


# ---------------------------------------------------------------------------------------------------------------------- the statistics
def test_stats_of_the_smallest_planes():
    rng = np.random.default_rng(4)
    cells = {(9, 9): 0, (9, 40): 0, (10, 10): 1, (10, 18): 2, (10, 26): 3, (18, 10): 2}
    for shape in SMALLEST:
        for interlaced in (False, True):
            got = _check_stats(stats_frames(rng, 1, *shape), 8, interlaced)
            assert got[:, :, 0].sum() == (0 if interlaced else cells[shape]), (shape, interlaced)          # (fields of at most 9 rows have no cell)
    assert not _check_stats(stats_frames(rng, 1, 1, 1)).any()
    assert _check_stats(np.random.default_rng(5).integers(0, 256, (1, 10, 24, 1)).astype(np.uint8))[:, :255, 0].sum() == 2          # the 8-byte form, its last cell on the plane's end


def test_stats_in_both_forms_and_over_tiles():
    """21 x 37 at an unaligned plane offset (a sample per access), 26 x 64 aligned (8 bytes and the dword behind them, the last cell
    ending with the allocation), one workgroup of cells plus ragged rests each way, field-wise with odd row counts."""
    rng = np.random.default_rng(5)
    assert _check_stats(stats_frames(rng, 1, 21, 37), off=1, before=5, after=2)[:, :255].any()
    assert _check_stats(stats_frames(rng, 1, 26, 64))[:, :255].any()
    assert _check_stats(stats_frames(rng, 1, 26, 64), before=8)[:, :255].any()
    tr, tc = stats_tile()
    for r, c in ((tr, tc), (tr, tc + 6), (tr + 5, tc + 14), (2 * tr + 3, tc + 22), (tr + 9, 2 * tc + 12)):
        for interlaced in (False, True):
            _check_stats(stats_frames(rng, 1, r, c), 8, interlaced)


@pytest.mark.parametrize("step", [1, 3, 4])
def test_stats_at_steps_and_depths(step):
    rng = np.random.default_rng(60 + step)
    for depth, cols, place in ((8, 48, {}), (8, 37, dict(off=1, before=5, after=3)), (10, 48, {}), (10, 40, dict(before=16)), (12, 48, {}),
                               (12, 37, dict(off=2, before=6, after=2))):
        m = stats_frames(rng, 1, 21, cols, step=step, depth=depth, above=True)
        assert depth == 8 or int(m.max()) > (1 << depth) - 1
        assert _check_stats(m, depth, step == 3, **place)[:, :255].any()


@pytest.mark.parametrize("rows", [19, 20, 21])
def test_stats_field_wise(rows):
    """19 rows: fields of 10 and 9 rows, the first has a cell and the second none; 20: both have one; 21: 11 and 10."""
    rng = np.random.default_rng(70 + rows)
    for cols, place in ((24, {}), (27, dict(off=1, before=3))):
        m = stats_frames(rng, 2, rows, cols)
        got = _check_stats(m, 8, True, **place)
        assert got[:, :, 0].sum() == 2 * (1 if rows == 19 else 2) * ((cols - 2) // 8)
        assert _check_stats(m, 8, False, **place)[:, :, 0].sum() == 2 * 2 * ((cols - 2) // 8)


def test_stats_frames_do_not_leak_and_calls_add():
    rng = np.random.default_rng(7)
    m = stats_frames(rng, 3, 26, 40)
    whole = _check_stats(m, 8, True)
    for k in range(3):
        assert np.array_equal(_stats(m[k:k + 1], 8, True), whole[k:k + 1])
    assert len({whole[k].tobytes() for k in range(3)}) == 3
    _check_stats(m, 8, False, calls=2)
    _check_stats(stats_frames(rng, 2, 23, 27, depth=12, above=True), 12, True, calls=2, off=2, before=4, after=2)


def test_the_special_cells():
    got = _check_stats(checkerboard(26, 34)[None, :, :, None])
    assert got[0, 254].tolist() == [12, 12 * 64 * 2040] and got[0, :254].sum() == 0 and got[0, 255].sum() == 0
    got = _check_stats(checkerboard(26, 32)[None, :, :, None])          # the 8-byte form
    assert got[0, 254].tolist() == [9, 9 * 64 * 2040]
    got = _check_stats(flat_beside_binned()[None, :, :, None])
    assert got[0, 255].tolist() == [1, 0] and got[0, :255, 0].sum() == 1
    got = _check_stats(np.full((2, 26, 32, 3), 200, np.uint8), 8, True)
    assert got[:, 255, 0].tolist() == [18, 18] and got[:, :255].sum() == 0


def test_entries_refuse_bad_arguments():
    lib = _lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    table = torch.zeros(2 * 512, dtype=torch.int64, device=DEV)
    p, q = buf.data_ptr(), table.data_ptr()
    s8, s16 = lib.savsr_video_noise_stats_u8, lib.savsr_video_noise_stats_u16
    bad = [
        # (frames, n_frames, frame_bytes, plane_offset, rows, cols, step[, depth], interlaced, out)
        (s8, (0, 2, 256, 0, 12, 12, 1, 0, q), "null pointer"),
        (s8, (p, 2, 256, 0, 12, 12, 1, 0, 0), "null pointer"),
        (s8, (p, 0, 256, 0, 12, 12, 1, 0, q), "n_frames >= 1"),
        (s8, (p, 2, 256, 0, 0, 12, 1, 0, q), "rows >= 1"),
        (s8, (p, 2, 256, 0, 12, 0, 1, 0, q), "a row holds at least one sample"),
        (s8, (p, 2, 256, 0, 12, 12, 0, 0, q), "step 1 .. 4"),
        (s8, (p, 2, 1024, 0, 12, 12, 5, 0, q), "step 1 .. 4"),
        (s8, (p, 2, 143, 0, 12, 12, 1, 0, q), "frame_bytes smaller than plane_offset plus the rows x row_bytes plane"),
        (s8, (p, 2, 256, 113, 12, 12, 1, 0, q), "frame_bytes smaller than plane_offset plus the rows x row_bytes plane"),
        (s8, (p, 2, 256, -1, 12, 12, 1, 0, q), "plane offsets >= 0"),
        (s8, (p, 2, 256, 0, 12, 12, 1, 2, q), "interlaced 0 or 1"),
        (s8, (p, 2, 256, 0, 12, 12, 1, -1, q), "interlaced 0 or 1"),
        (s8, (p, 2, 256, 0, 12, 12, 1, 0, q + 4), "out must be 8-byte aligned"),
        (s8, (p, 1, 1 << 40, 0, 1 << 20, 1 << 20, 1, 0, q), "a plane of at most 2147418112 bytes"),
        (s16, (p, 2, 512, 0, 12, 12, 1, 8, 0, q), "depth 10 or 12 (8 bits: savsr_video_noise_stats_u8)"),
        (s16, (p, 2, 512, 0, 12, 12, 1, 11, 0, q), "depth 10 or 12"),
        (s16, (p + 1, 2, 512, 0, 12, 12, 1, 10, 0, q), "2-byte aligned"),
        (s16, (p, 2, 513, 0, 12, 12, 1, 10, 0, q), "2-byte aligned"),
        (s16, (p, 2, 512, 3, 12, 12, 1, 12, 0, q), "2-byte aligned"),
        (s16, (p, 2, 287, 0, 12, 12, 1, 12, 0, q), "frame_bytes smaller"),
        (s16, (p, 2, 512, 0, 12, 12, 1, 12, 2, q), "interlaced 0 or 1"),
    ]
    for fn, args, words in bad:
        assert fn(*args, None) == -1, (fn.__name__, args)          # SAVSR_E_ARG
        msg = lib.savsr_last_error().decode()
        assert words in msg and fn.__name__[len("savsr_"):] + ":" in msg, (fn.__name__, args, msg)
    torch.cuda.synchronize()
    assert not table.any()          # refused before the device is touched: no launch left behind


# ---------------------------------------------------------------------------------------------------------------------- the python surface
def test_noise_stats_and_estimate_noise_of_frame_kinds():
    rng = np.random.default_rng(8)
    v = stats_frames(rng, 2, 27, 35, step=3)
    for interlaced in (False, True):
        got = savsr_amd.noise_stats(torch.from_numpy(v), interlaced=interlaced)
        assert got.device.type == "cuda" and got.dtype == torch.int64 and got.shape == (2, 2, 256, 2)
        assert np.array_equal(got.cpu().numpy(), NZ.noise_stats_frames(v, interlaced=interlaced))
    from savsr_amd import yuv
    for fmt, layout, depth, (h, w) in (("i420", "420", 8, (44, 56)), ("i444", "444", 12, (20, 34)), ("y400", "400", 10, (21, 33))):
        sizes = [(h, w)] + ([] if layout == "400" else [yuv.chroma_hw(h, w, layout)] * 2)
        frames = np.ascontiguousarray(np.concatenate([as_bytes(stats_frames(rng, 3, *hw, depth=depth, above=True)) for hw in sizes], 1))
        for interlaced in (False, True):
            got = savsr_amd.noise_stats(torch.from_numpy(frames), fmt, (h, w), depth, interlaced)
            want = NZ.noise_stats_frames(frames, fmt, (h, w), depth, interlaced)
            assert np.array_equal(got.cpu().numpy(), want) and want[:, 0].any() and want[:, 1].any() == (layout != "400")
        got = savsr_amd.estimate_noise(torch.from_numpy(frames).to(DEV), fmt, (h, w), depth, min_cells=4, quantile=0.5, floor=0)
        want = NZ.verdict_from_stats(NZ.noise_stats_frames(frames, fmt, (h, w), depth).sum(0), 0.5, 4, 0)
        assert got.sigma == want.sigma and got.chroma_sigma == want.chroma_sigma and got.cells == want.cells and got.flat == want.flat
        assert np.array_equal(got.table, want.table) and got.sigma is not None and (got.chroma_sigma is None) == (layout == "400")
    with pytest.raises(ValueError, match="float frames have no integer samples to measure noise in"):
        savsr_amd.noise_stats(torch.zeros(3, 3, 12, 12, device=DEV))
    with pytest.raises(ValueError, match="float frames have no integer samples to measure noise in"):
        savsr_amd.estimate_noise(torch.zeros(3, 3, 12, 12, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------- end to end
H, W, N = 48, 64, 5
NOISY_KEY = 3          # (the sigma = 2 video whose estimate maps to a spatial strength other than the default 3.0: chosen on the specification)


def _video(key, sigma, n=N, h=H, w=W, c=3):
    """[n, h, w, c] uint8: every channel of every frame the picture with noise of its own seed."""
    return torch.from_numpy(np.stack([np.stack([picture(case_seed(key, t, ch), h, w, sigma) for ch in range(c)], -1) for t in range(n)]))


def test_spatial_auto_is_the_explicit_call(net3):
    v = _video(NOISY_KEY, 2.0)
    verdict = savsr_amd.estimate_noise(v)
    want = NZ.estimate_noise_frames(v.numpy())
    assert verdict.sigma == want.sigma and np.array_equal(verdict.table, want.table) and verdict.chroma_sigma is None
    kw = verdict.spatial_kwargs()
    assert abs(float(verdict.sigma) / np.sqrt(4 + 1 / 12) - 1) <= 0.10 and set(kw) == {"spatial_strength"} and kw["spatial_strength"] != 3.0
    got = net3.upscale_video(v, scale=2, out="uint8", spatial_denoise="nlm", spatial_strength="auto")
    assert torch.equal(got, net3.upscale_video(v, scale=2, out="uint8", spatial_denoise="nlm", **kw))
    assert not torch.equal(got, net3.upscale_video(v, scale=2, out="uint8", spatial_denoise="nlm"))
    assert not torch.equal(got, net3.upscale_video(v, scale=2, out="uint8"))


def test_auto_leaves_a_noise_free_video_alone(net3):
    v = _video(9, 0.0)
    verdict = savsr_amd.estimate_noise(v)
    assert verdict.sigma is not None and verdict.sigma < NZ.DEFAULT_FLOOR and verdict.spatial_kwargs() == {} and verdict.denoise_kwargs() == {}
    plain = net3.upscale_video(v, scale=2, out="uint8")
    assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", spatial_denoise="nlm", spatial_strength="auto"), plain)
    assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", denoise="ata", denoise_strength="auto"), plain)
    assert not torch.equal(net3.upscale_video(v, scale=2, out="uint8", spatial_denoise="nlm"), plain)


def test_temporal_auto_is_the_explicit_call(net3):
    v = _video(NOISY_KEY, 2.0)
    kw = savsr_amd.estimate_noise(v).denoise_kwargs()
    assert set(kw) == {"denoise_strength"} and kw["denoise_strength"] != (4, 9) and kw == NZ.estimate_noise_frames(v.numpy()).denoise_kwargs()
    got = net3.upscale_video(v, scale=2, out="uint8", denoise="ata", denoise_strength="auto", denoise_radius=2)
    assert torch.equal(got, net3.upscale_video(v, scale=2, out="uint8", denoise="ata", denoise_radius=2, **kw))
    assert not torch.equal(got, net3.upscale_video(v, scale=2, out="uint8", denoise="ata", denoise_radius=2))
    assert not torch.equal(got, net3.upscale_video(v, scale=2, out="uint8"))


def test_both_autos_measure_where_their_stages_read(net3):
    """The spatial estimate is taken on the temporally denoised frames: the two stages by hand."""
    v = _video(NOISY_KEY, 2.0)
    first = savsr_amd.estimate_noise(v)
    kw_t = first.denoise_kwargs()
    calm = savsr_amd.denoise_video(v, strength=kw_t["denoise_strength"])
    second = savsr_amd.estimate_noise(calm)
    kw_s = second.spatial_kwargs()
    assert second.sigma < first.sigma and kw_s and kw_s != first.spatial_kwargs()
    got = net3.upscale_video(v, scale=2, out="uint8", denoise="ata", denoise_strength="auto", spatial_denoise="nlm", spatial_strength="auto")
    assert torch.equal(got, net3.upscale_video(v, scale=2, out="uint8", denoise="ata", spatial_denoise="nlm", **kw_t, **kw_s))
    assert torch.equal(got, net3.upscale_video(savsr_amd.denoise_spatial(calm, strength=kw_s["spatial_strength"]), scale=2, out="uint8"))
    assert not torch.equal(got, net3.upscale_video(v, scale=2, out="uint8", denoise="ata", spatial_denoise="nlm", **kw_t, **first.spatial_kwargs()))


def test_spatial_auto_measures_the_cropped_frames(net3):
    rect = (8, 8, 32, 48)
    v = _video(10, 8.0)
    v[:, 8:40, 8:56] = _video(0, 2.0)[:, 8:40, 8:56]          # loud noise around a quieter picture
    inside = savsr_amd.estimate_noise(v[:, 8:40, 8:56].contiguous()).spatial_kwargs()
    assert inside and inside != savsr_amd.estimate_noise(v).spatial_kwargs()
    for bars in ("keep", "drop"):
        got = net3.upscale_video(v, scale=2, out="uint8", crop=rect, bars=bars, spatial_denoise="nlm", spatial_strength="auto")
        assert torch.equal(got, net3.upscale_video(v, scale=2, out="uint8", crop=rect, bars=bars, spatial_denoise="nlm", **inside))
    assert not torch.equal(got, net3.upscale_video(v, scale=2, out="uint8", crop=rect, bars="drop", spatial_denoise="nlm",
                                                   **savsr_amd.estimate_noise(v).spatial_kwargs()))


def test_an_explicit_chroma_strength_wins(net3):
    h, w = 64, 96
    planes = [np.stack([picture(case_seed(20 + i, t), *hw, s) for t in range(N)]).reshape(N, -1)
              for i, (hw, s) in enumerate((((h, w), 2.0), ((h // 2, w // 2), 1.0), ((h // 2, w // 2), 1.0)))]
    v = torch.from_numpy(np.ascontiguousarray(np.concatenate(planes, 1)))
    fmt = dict(scale=2, out="i420", pixel_format="i420", size=(h, w))
    verdict = savsr_amd.estimate_noise(v, "i420", (h, w))
    kw = verdict.spatial_kwargs()
    assert set(kw) == {"spatial_strength", "spatial_chroma_strength"} and kw["spatial_chroma_strength"] < kw["spatial_strength"]
    got = net3.upscale_video(v, spatial_denoise="nlm", spatial_strength="auto", **fmt)
    assert torch.equal(got, net3.upscale_video(v, spatial_denoise="nlm", **kw, **fmt))
    given = net3.upscale_video(v, spatial_denoise="nlm", spatial_strength="auto", spatial_chroma_strength=6.0, **fmt)
    assert torch.equal(given, net3.upscale_video(v, spatial_denoise="nlm", spatial_strength=kw["spatial_strength"], spatial_chroma_strength=6.0, **fmt))
    assert not torch.equal(given, got)


# ---------------------------------------------------------------------------------------------------------------------- the CLI
def test_cli_auto_strengths_on_a_y4m_file(net3, tmp_path, capsys):
    """--denoise-strength auto and --spatial-strength auto on a small 4:2:0 file: one line on stderr per pass with the verdict and the
    equivalent flags, the JSON report, and the bytes of upscale_video with both "auto"; a noise-free file gives the bytes of the call
    without the stages."""
    import io
    import json

    from savsr_amd import io as sio
    from savsr_amd import y4m
    from savsr_amd.upscale import main
    h, w = 64, 96
    ckpt = tmp_path / "net.pth"
    sio.save_network(net3, str(ckpt))
    fmt = dict(scale=2, out="i420", pixel_format="i420", size=(h, w))
    for name, sigma in (("noisy", 2.0), ("clean", 0.0)):
        planes = [np.stack([picture(case_seed(30 + i, t), *hw, sigma) for t in range(N)]).reshape(N, -1)
                  for i, hw in enumerate(((h, w), (h // 2, w // 2), (h // 2, w // 2)))]
        frames = np.ascontiguousarray(np.concatenate(planes, 1))
        f = io.BytesIO()
        y4m.Y4MWriter(f, w, h, (25, 1), "p", (1, 1)).write(frames)
        src, dst, out = tmp_path / f"{name}.y4m", tmp_path / f"{name}_sr.y4m", tmp_path / f"{name}.json"
        src.write_bytes(f.getvalue())
        assert main(["-i", str(src), "-o", str(dst), "--scale", "2", "--checkpoint", str(ckpt), "--chunk", "2", "--denoise", "ata", "--denoise-radius", "2",
                     "--denoise-strength", "auto", "--spatial-denoise", "nlm", "--spatial-strength", "auto", "--noise-out", str(out)]) == 0
        err = capsys.readouterr().err
        v = torch.from_numpy(frames)
        want = net3.upscale_video(v, denoise="ata", denoise_radius=2, denoise_strength="auto", spatial_denoise="nlm", spatial_strength="auto", **fmt)
        g = io.BytesIO()
        y4m.Y4MWriter(g, 2 * w, 2 * h, (25, 1), "p", y4m.scaled_aspect((1, 1), (h, w), (2 * h, 2 * w))).write(want.cpu().numpy())
        assert dst.read_bytes() == g.getvalue(), name
        report = json.loads(out.read_text())
        first = savsr_amd.estimate_noise(v, "i420", (h, w))
        assert report["denoise"]["sigma"]["fraction"] == [first.sigma.numerator, first.sigma.denominator]
        assert report["denoise"]["cells"] == list(first.cells) and report["denoise"]["table"] == first.table.tolist()
        if sigma:
            kw_t = first.denoise_kwargs()
            (a, b), (ca, cb) = kw_t["denoise_strength"], kw_t["denoise_chroma_strength"]
            flags = f"--denoise ata --denoise-strength {a},{b} --denoise-chroma-strength {ca},{cb}"
            assert f"--denoise-strength auto: sigma {float(first.sigma):.3f} from {first.cells[0]} cells" in err and flags in err
            assert report["denoise"]["flags"] == flags
            second = savsr_amd.estimate_noise(savsr_amd.denoise_video(v, "i420", (h, w), 8, 2, (a, b), (ca, cb)), "i420", (h, w))
            kw_s = second.spatial_kwargs()
            flags = f"--spatial-denoise nlm --spatial-strength {kw_s['spatial_strength']:g} --spatial-chroma-strength {kw_s['spatial_chroma_strength']:g}"
            assert "--spatial-strength auto: sigma" in err and flags in err and report["spatial"]["flags"] == flags
            assert report["spatial"]["table"] == second.table.tolist()
            assert torch.equal(want, net3.upscale_video(v, denoise="ata", denoise_radius=2, spatial_denoise="nlm", **kw_t, **kw_s, **fmt))
            assert not torch.equal(want, net3.upscale_video(v, **fmt))
        else:
            assert "--denoise-strength auto" in err and "--denoise none" in err and "--spatial-denoise none" in err
            assert report["denoise"]["flags"] == "--denoise none" and report["spatial"]["flags"] == "--spatial-denoise none"
            assert torch.equal(want, net3.upscale_video(v, **fmt))
