"""GPU checks of the deblocker's grid origin and of the grid detector: savsr_video_deblock_u8_o / _u16_o and savsr_video_grid_stats_u8 /
_u16 against the numpy specifications bit for bit (savsr_amd/deblock.py with an origin, savsr_amd/grid.py), at the smallest shapes at
which the kernels can go wrong (tests/grid_cases.py, tests/deblock_cases.py), the entries' refusals, and the properties of
upscale_video(deblock_origin=..., deblock_grid="auto")."""
import numpy as np
import pytest
import torch

import savsr_amd
from savsr_amd import grid as G
from savsr_amd.deblock import deblock_frames, deblock_plane
from savsr_amd.utils import synth
from tests.deblock_cases import COVER_SHAPE, as_bytes, case_frames, one_tile_plus, two_tiles_ragged
from tests.grid_cases import blocky, case_seed, stats_frames, stats_tile
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


def _place(m, off, before, after):
    """The samples [N, R, C, step] as the plane `before` bytes into frames of before + plane + after bytes, the first frame `off` bytes
    past a 256-byte aligned allocation: (the device buffer, frame bytes, plane bytes)."""
    n = m.shape[0]
    plane = as_bytes(m)
    fb = before + plane.shape[1] + after
    host = np.full((n, fb), 0x3C, np.uint8)
    host[:, before:before + plane.shape[1]] = plane
    src = torch.empty(n * fb + off + 64, dtype=torch.uint8, device=DEV)
    assert src.data_ptr() % 256 == 0
    src[off:off + n * fb].copy_(torch.from_numpy(host).reshape(-1))
    return src, fb, plane.shape[1]


# ---------------------------------------------------------------------------------------------------------------------- deblock with an origin
def _deblock(m, depth=8, block=8, mode="weak", interlaced=False, origin=(0, 0), off=0, before=0, after=0, old=False):
    """savsr_video_deblock_*_o (old: the entry without an origin) into poisoned output followed by guard bytes: [N, R, C, step]."""
    n, r, c, step = m.shape
    src, fb, pb = _place(m, off, before, after)
    dst = torch.full((n * fb + off + 64,), POISON, dtype=torch.uint8, device=DEV)
    lib, st, sh = _lib(), torch.cuda.current_stream().cuda_stream, depth - 8
    head = (src.data_ptr() + off, n, fb, before, r, c, step) + ((depth,) if depth > 8 else ())
    tail = (block, int(mode == "strong"), int(interlaced), 25 << sh, 13 << sh, dst.data_ptr() + off, fb, before) + (() if old else tuple(origin)) + (st,)
    name = ("savsr_video_deblock_u16" if depth > 8 else "savsr_video_deblock_u8") + ("" if old else "_o")
    assert getattr(lib, name)(*head, *tail) == 0, lib.savsr_last_error()
    got = dst.cpu().numpy()
    assert (got[:off] == POISON).all() and (got[off + n * fb:] == POISON).all()
    got = got[off:off + n * fb].reshape(n, fb)
    assert (got[:, :before] == POISON).all() and (got[:, before + pb:] == POISON).all()
    got = np.ascontiguousarray(got[:, before:before + pb])
    return got.view("<u2").reshape(m.shape) if depth > 8 else got.reshape(m.shape)


def _check_deblock(m, depth=8, block=8, mode="weak", interlaced=False, origin=(0, 0), **place):
    got = _deblock(m, depth, block, mode, interlaced, origin, **place)
    want = np.empty_like(m)
    for t in range(m.shape[0]):
        for ch in range(m.shape[3]):
            want[t, :, :, ch] = deblock_plane(m[t, :, :, ch], depth, block, mode, (25, 13), interlaced, origin)
    assert np.array_equal(got, want), (m.shape, depth, block, mode, interlaced, origin, place, np.argwhere(got != want)[:4].tolist())
    return got


def test_every_origin_of_block_8_and_the_corner_origins_of_4_and_16():
    rng = np.random.default_rng(1)
    m = case_frames(rng, 1, *COVER_SHAPE)
    seen = set()
    for oy in range(8):
        for ox in range(8):
            seen.add(_check_deblock(m, 8, 8, "strong", False, (oy, ox)).tobytes())
            if oy % 2 == 0:
                _check_deblock(m, 8, 8, "weak", True, (oy, ox))
    assert len(seen) == 64          # every origin filters other samples
    for block in (4, 16):
        for o in ((1, 1), (block - 1, block - 1)):
            _check_deblock(case_frames(rng, 1, *COVER_SHAPE, block=block), 8, block, "strong", False, o)


def test_planes_whose_p_side_lies_beyond_them():
    rng = np.random.default_rng(2)
    for r, c in ((1, 1), (2, 9), (9, 2)):
        for mode in ("weak", "strong"):
            _check_deblock(case_frames(rng, 1, r, c), 8, 8, mode, False, (1, 1))


@pytest.mark.parametrize("interlaced", [False, True])
@pytest.mark.parametrize("mode", ["weak", "strong"])
@pytest.mark.parametrize("depth", [8, 12])
@pytest.mark.parametrize("step", [1, 3, 4])
def test_tiles_at_an_origin(step, depth, mode, interlaced):
    """One tile plus a row and a column and two ragged tiles each way: the tile grid starts before the plane, and a misaligned plane
    inside a frame keeps the bytes around it."""
    rng = np.random.default_rng(100 * step + 2 * depth + 50 * (mode == "strong") + interlaced)
    for shape in (one_tile_plus(step), two_tiles_ragged(step)):
        for o in ((1, 1), (7, 5)):
            o = (o[0] - o[0] % 2, o[1]) if interlaced else o
            m = case_frames(rng, 1, *shape, step=step, depth=depth, above=True)
            assert not np.array_equal(_check_deblock(m, depth, 8, mode, interlaced, o, off=2, before=6, after=2), m)


def test_the_old_entries_are_the_new_ones_at_origin_zero():
    rng = np.random.default_rng(3)
    for depth, step, interlaced in ((8, 1, False), (8, 3, True), (10, 1, True), (12, 2, False)):
        m = case_frames(rng, 2, *two_tiles_ragged(step), step=step, depth=depth, above=True)
        for mode in ("weak", "strong"):
            a = _deblock(m, depth, 8, mode, interlaced, old=True, off=2, before=4, after=2)
            assert np.array_equal(a, _check_deblock(m, depth, 8, mode, interlaced, (0, 0), off=2, before=4, after=2))


# ---------------------------------------------------------------------------------------------------------------------- grid statistics
def _stats(m, depth=8, interlaced=False, cap=32, off=0, before=0, after=0, calls=1):
    """savsr_video_grid_stats_* `calls` times on one zeroed table between guard cells: int64 [N, 2, 16]."""
    n, r, c, step = m.shape
    src, fb, _ = _place(m, off, before, after)
    out = torch.full((n * 32 + 16,), -7, dtype=torch.int64, device=DEV)
    out[8:8 + n * 32] = 0
    lib, st = _lib(), torch.cuda.current_stream().cuda_stream
    head = (src.data_ptr() + off, n, fb, before, r, c, step) + ((depth,) if depth > 8 else ())
    fn = lib.savsr_video_grid_stats_u16 if depth > 8 else lib.savsr_video_grid_stats_u8
    for _ in range(calls):
        assert fn(*head, int(interlaced), cap, out.data_ptr() + 64, st) == 0, lib.savsr_last_error()
    got = out.cpu().numpy()
    assert (got[:8] == -7).all() and (got[8 + n * 32:] == -7).all()
    return got[8:8 + n * 32].reshape(n, 2, 16)


def _check_stats(m, depth=8, interlaced=False, cap=32, calls=1, **place):
    got = _stats(m, depth, interlaced, cap, calls=calls, **place)
    want = np.stack([sum(G.grid_stats_matrix(m[t, :, :, ch], depth, interlaced, cap) for ch in range(m.shape[3])) for t in range(m.shape[0])]) * calls
    assert np.array_equal(got, want), (m.shape, depth, interlaced, cap, place, np.argwhere(got != want)[:4].tolist())
    return got


def test_stats_of_the_smallest_planes():
    rng = np.random.default_rng(4)
    for interlaced in (False, True):
        assert not _check_stats(stats_frames(rng, 1, 1, 1), 8, interlaced).any()
        assert not _check_stats(stats_frames(rng, 1, 3, 3), 8, interlaced).any()
    m = np.array([[10, 10, 14, 14]] * 4, np.uint8)          # 4 x 4: one boundary each way; the rows' is a hit in every row
    got = _check_stats(np.ascontiguousarray(m[None, :, :, None]))
    assert got[0, 0].tolist() == [0, 0, 4] + [0] * 13 and not got[0, 1].any()
    got = _check_stats(np.ascontiguousarray(m.T[None, :, :, None]))
    assert got[0, 1].tolist() == [0, 0, 4] + [0] * 13 and not got[0, 0].any()


def test_stats_in_both_forms_and_over_tiles():
    """5 x 37 at an unaligned plane offset (a sample per access), 8 x 64 aligned (16-byte loads), one band / one workgroup of the
    16-byte form plus ragged rests each way, field-wise with odd row counts."""
    rng = np.random.default_rng(5)
    assert _check_stats(stats_frames(rng, 1, 5, 37), off=1, before=3, after=2).any()
    assert _check_stats(stats_frames(rng, 1, 8, 64)).any()
    tr, tc = stats_tile()
    for r, c in ((tr + 1, 64), (2 * tr + 5, 80), (tr, tc + 16), (tr + 3, 2 * tc + 48), (2 * tr + 3, tc + 21)):
        for interlaced in (False, True):
            _check_stats(stats_frames(rng, 1, r, c), 8, interlaced)
    _check_stats(stats_frames(rng, 1, 7, 48), 8, True)
    _check_stats(stats_frames(rng, 1, 2, 48), 8, True)


@pytest.mark.parametrize("step", [1, 3, 4])
def test_stats_at_steps_and_depths(step):
    rng = np.random.default_rng(60 + step)
    for depth, cols, place in ((8, 48, {}), (8, 37, dict(off=1, before=5, after=3)), (10, 48, {}), (12, 37, dict(off=2, before=6, after=2))):
        assert _check_stats(stats_frames(rng, 1, 21, cols, step=step, depth=depth, above=True), depth, step == 3, **place).any()
    for cap in (0, 1, 255):
        _check_stats(stats_frames(rng, 1, 19, 48, step=step), 8, False, cap)


def test_stats_frames_do_not_leak_and_calls_add():
    rng = np.random.default_rng(7)
    m = stats_frames(rng, 3, 18, 32)
    whole = _check_stats(m, 8, True)
    for k in range(3):
        assert np.array_equal(_stats(m[k:k + 1], 8, True), whole[k:k + 1])
    assert len({whole[k].tobytes() for k in range(3)}) == 3
    _check_stats(m, 8, False, calls=2)
    _check_stats(stats_frames(rng, 2, 7, 23, depth=12, above=True), 12, True, calls=2, off=2, before=4, after=2)


def test_entries_refuse_bad_arguments():
    lib = _lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    out = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    cells = torch.zeros(64, dtype=torch.int64, device=DEV)
    p, o, q = buf.data_ptr(), out.data_ptr(), cells.data_ptr()
    s8, s16, d8, d16 = lib.savsr_video_grid_stats_u8, lib.savsr_video_grid_stats_u16, lib.savsr_video_deblock_u8_o, lib.savsr_video_deblock_u16_o
    bad = [
        # (frames, n_frames, frame_bytes, plane_offset, rows, cols, step[, depth], interlaced, cap, out)
        (s8, (0, 2, 64, 0, 8, 8, 1, 0, 32, q), "null pointer"),
        (s8, (p, 2, 64, 0, 8, 8, 1, 0, 32, 0), "null pointer"),
        (s8, (p, 0, 64, 0, 8, 8, 1, 0, 32, q), "n_frames >= 1"),
        (s8, (p, 2, 64, 0, 0, 8, 1, 0, 32, q), "rows >= 1"),
        (s8, (p, 2, 64, 0, 8, 0, 1, 0, 32, q), "at least one sample"),
        (s8, (p, 2, 64, 0, 8, 8, 0, 0, 32, q), "step 1 .. 4"),
        (s8, (p, 2, 64, 0, 8, 8, 5, 0, 32, q), "step 1 .. 4"),
        (s8, (p, 2, 63, 0, 8, 8, 1, 0, 32, q), "frame_bytes smaller"),
        (s8, (p, 2, 64, 1, 8, 8, 1, 0, 32, q), "frame_bytes smaller"),
        (s8, (p, 2, 64, -1, 8, 8, 1, 0, 32, q), "plane offsets >= 0"),
        (s8, (p, 2, 64, 0, 8, 8, 1, 0, 32, q + 4), "out must be 8-byte aligned"),
        (s8, (p, 2, 64, 0, 8, 8, 1, 2, 32, q), "interlaced 0 or 1"),
        (s8, (p, 2, 64, 0, 8, 8, 1, 0, -1, q), "cap 0 .. 255"),
        (s8, (p, 2, 64, 0, 8, 8, 1, 0, 256, q), "cap 0 .. 255"),
        (s16, (p, 2, 128, 0, 8, 8, 1, 8, 0, 32, q), "depth 10 or 12 (8 bits: savsr_video_grid_stats_u8)"),
        (s16, (p + 1, 2, 128, 0, 8, 8, 1, 10, 0, 32, q), "2-byte aligned"),
        (s16, (p, 2, 129, 0, 8, 8, 1, 10, 0, 32, q), "2-byte aligned"),
        (s16, (p, 2, 130, 1, 8, 8, 1, 12, 0, 32, q), "2-byte aligned"),
        # (frames, n_frames, frame_bytes, plane_offset, rows, cols, step[, depth], block, strong, interlaced, thr_a, thr_b, out, out_frame_bytes, out_plane_offset, oy, ox)
        (d8, (p, 2, 64, 0, 8, 8, 1, 8, 0, 0, 25, 13, o, 64, 0, 8, 0), "origin_y and origin_x 0 .. block - 1"),
        (d8, (p, 2, 64, 0, 8, 8, 1, 8, 0, 0, 25, 13, o, 64, 0, 0, -1), "origin_y and origin_x 0 .. block - 1"),
        (d8, (p, 2, 64, 0, 8, 8, 1, 4, 0, 0, 25, 13, o, 64, 0, 0, 4), "origin_y and origin_x 0 .. block - 1"),
        (d8, (p, 2, 64, 0, 8, 8, 1, 8, 0, 1, 25, 13, o, 64, 0, 3, 0), "origin_y even with interlaced"),
        (d8, (p, 2, 64, 0, 8, 8, 1, 12, 0, 0, 25, 13, o, 64, 0, 0, 0), "block 4, 8 or 16"),
        (d8, (0, 2, 64, 0, 8, 8, 1, 8, 0, 0, 25, 13, o, 64, 0, 1, 1), "null pointer"),
        (d16, (p, 2, 128, 0, 8, 8, 1, 10, 16, 0, 0, 25, 13, o, 128, 0, 16, 0), "origin_y and origin_x 0 .. block - 1"),
        (d16, (p, 2, 128, 0, 8, 8, 1, 12, 8, 0, 1, 25, 13, o, 128, 0, 1, 1), "origin_y even with interlaced"),
        (d16, (p, 2, 128, 0, 8, 8, 1, 8, 8, 0, 0, 25, 13, o, 128, 0, 1, 1), "depth 10 or 12 (8 bits: savsr_video_deblock_u8_o)"),
    ]
    for fn, args, words in bad:
        assert fn(*args, None) == -1, (fn.__name__, args)          # SAVSR_E_ARG
        msg = lib.savsr_last_error().decode()
        assert words in msg and fn.__name__[len("savsr_"):] + ":" in msg, (fn.__name__, args, msg)
    torch.cuda.synchronize()
    assert not out.any() and not cells.any()          # refused before the device is touched: no launch left behind


# ---------------------------------------------------------------------------------------------------------------------- the python surface
def test_grid_stats_and_deblock_video_of_frame_kinds():
    rng = np.random.default_rng(8)
    v = stats_frames(rng, 2, 19, 27, step=3)
    for interlaced in (False, True):
        got = savsr_amd.grid_stats(torch.from_numpy(v), interlaced=interlaced)
        assert got.device.type == "cuda" and got.dtype == torch.int64 and got.shape == (2, 2, 2, 16)
        assert np.array_equal(got.cpu().numpy(), G.grid_stats_frames(v, interlaced=interlaced))
    from savsr_amd import yuv
    for fmt, layout, depth, (h, w) in (("i420", "420", 8, (20, 38)), ("i444", "444", 12, (12, 18)), ("y400", "400", 10, (9, 33))):
        sizes = [(h, w)] + ([] if layout == "400" else [yuv.chroma_hw(h, w, layout)] * 2)
        frames = np.ascontiguousarray(np.concatenate([as_bytes(stats_frames(rng, 3, *hw, depth=depth)) for hw in sizes], 1))
        got = savsr_amd.grid_stats(torch.from_numpy(frames), fmt, (h, w), depth, True, cap=20)
        want = G.grid_stats_frames(frames, fmt, (h, w), depth, True, 20)
        assert np.array_equal(got.cpu().numpy(), want) and want[:, 0].any() and want[:, 1].any() == (layout != "400")
        co = None if layout != "420" else (4, 6)
        got = savsr_amd.deblock_video(torch.from_numpy(frames), fmt, (h, w), depth, 8, "strong", (25, 13), (60, 30), True, (2, 5), co)
        assert np.array_equal(got.cpu().numpy(), deblock_frames(frames, fmt, (h, w), depth, 8, "strong", (25, 13), (60, 30), True, (2, 5), co))
    got = savsr_amd.deblock_video(torch.from_numpy(v), origin=(3, 5))
    assert np.array_equal(got.cpu().numpy(), deblock_frames(v, origin=(3, 5))) and not np.array_equal(got.cpu().numpy(), deblock_frames(v))
    with pytest.raises(ValueError, match="float frames have no integer samples to find a grid in"):
        savsr_amd.grid_stats(torch.zeros(3, 3, 4, 4, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------- end to end
H, W, N = 96, 128, 7
KW = dict(deblock="strong", deblock_strength=(40, 20))


def _video(block, origin, sigma=1.0, n=N, c=3, key=0):
    """[n, H, W, c] uint8: every channel of every frame a blocky picture of its own seed (block None: unblocked)."""
    v = np.stack([np.stack([blocky(case_seed(key, t, ch), H, W, block, 6, sigma, origin) for ch in range(c)], -1) for t in range(n)])
    return torch.from_numpy(v)


def test_upscale_video_with_an_origin_is_the_call_on_the_filtered_video(net3):
    v = _video(8, (3, 5), n=5)[:, :24, :32].contiguous()
    clean = savsr_amd.deblock_video(v, mode="strong", strength=(40, 20), origin=(3, 5))
    assert not torch.equal(clean, savsr_amd.deblock_video(v, mode="strong", strength=(40, 20)))
    want = net3.upscale_video(clean, scale=2, out="uint8")
    got = net3.upscale_video(v, scale=2, out="uint8", deblock_origin=(3, 5), **KW)
    assert torch.equal(got, want) and not torch.equal(got, net3.upscale_video(v, scale=2, out="uint8", **KW))
    by_field = savsr_amd.deblock_video(v, mode="strong", strength=(40, 20), interlaced=True, origin=(2, 5))
    assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", fields="tff", field_rate="same", deblock_origin=(2, 5), **KW),
                       net3.upscale_video(by_field, scale=2, out="uint8", fields="tff", field_rate="same"))
    from savsr_amd import VideoUpscaler
    up = VideoUpscaler(net3, 2, out="uint8", deblock_origin=(3, 5), **KW)
    assert torch.equal(torch.cat([up.push(v[:2]), up.push(v[2:]), up.finish()], 0), want)


def test_grid_auto_is_the_explicit_call_on_a_blocky_video(net3):
    v = _video(8, (3, 5), key=1)
    verdict = savsr_amd.detect_grid(v)
    assert verdict.block == 8 and verdict.origin == (3, 5) and verdict.chroma_origin is None
    assert verdict.kwargs() == dict(deblock_block=8, deblock_origin=(3, 5))
    assert np.array_equal(verdict.table, G.grid_stats_frames(v.numpy()).sum(0))
    got = net3.upscale_video(v, scale=2, out="uint8", deblock_grid="auto", **KW)
    assert torch.equal(got, net3.upscale_video(v, scale=2, out="uint8", **verdict.kwargs(), **KW))
    assert not torch.equal(got, net3.upscale_video(v, scale=2, out="uint8", **KW))
    assert not torch.equal(got, net3.upscale_video(v, scale=2, out="uint8"))


def test_grid_auto_leaves_an_unblocked_video_alone(net3):
    v = _video(None, (0, 0), key=2)
    verdict = savsr_amd.detect_grid(v)
    assert verdict.block is None and verdict.kwargs() == {}
    plain = net3.upscale_video(v, scale=2, out="uint8")
    assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", deblock_grid="auto", **KW), plain)
    assert not torch.equal(net3.upscale_video(v, scale=2, out="uint8", **KW), plain)


# ---------------------------------------------------------------------------------------------------------------------- the CLI
def test_cli_grid_auto_on_a_y4m_file(net3, tmp_path, capsys):
    """--deblock-grid auto on a 4:2:0 file whose luma grid sits at (3, 5) and whose chroma planes are unblocked: one line on stderr with
    the verdict and the equivalent flags, the JSON verdict, and the bytes of upscale_video(deblock_grid="auto") -- which leaves the chroma
    planes alone; an unblocked file gives the bytes of the call without the stage."""
    import io
    import json

    from savsr_amd import io as sio
    from savsr_amd import y4m
    from savsr_amd.upscale import main
    ckpt = tmp_path / "net.pth"
    sio.save_network(net3, str(ckpt))
    fmt = dict(scale=2, out="i420", pixel_format="i420", size=(H, W))
    for name, block in (("blocky", 8), ("clean", None)):
        luma = np.stack([blocky(case_seed(3, t), H, W, block, 6, 1.0, (3, 5)) for t in range(N)]).reshape(N, -1)
        chroma = np.stack([blocky(case_seed(4, t), H, W // 2, None, 0, 1.0) for t in range(N)]).reshape(N, -1)          # Cb then Cr: two H / 2 x W / 2 planes
        frames = np.ascontiguousarray(np.concatenate([luma, chroma], 1))
        f = io.BytesIO()
        y4m.Y4MWriter(f, W, H, (25, 1), "p", (1, 1)).write(frames)
        src, dst, out = tmp_path / f"{name}.y4m", tmp_path / f"{name}_sr.y4m", tmp_path / f"{name}.json"
        src.write_bytes(f.getvalue())
        assert main(["-i", str(src), "-o", str(dst), "--scale", "2", "--checkpoint", str(ckpt), "--chunk", "3", "--deblock", "strong",
                     "--deblock-strength", "40,20", "--deblock-grid", "auto", "--grid-out", str(out)]) == 0
        err = capsys.readouterr().err
        v = torch.from_numpy(frames)
        want = net3.upscale_video(v, deblock_grid="auto", **fmt, **KW)
        g = io.BytesIO()
        y4m.Y4MWriter(g, 2 * W, 2 * H, (25, 1), "p", y4m.scaled_aspect((1, 1), (H, W), (2 * H, 2 * W))).write(want.cpu().numpy())
        assert dst.read_bytes() == g.getvalue(), name
        found = json.loads(out.read_text())
        if block:
            assert "--deblock-grid auto: block 8 at origin 3,5: --deblock-block 8 --deblock-origin 3,5 --deblock-chroma-origin 0,0 --deblock-chroma-strength 0,0" in err
            assert "--deblock strong: block 8 at origin 3,5 (chroma 0,0), strength 40,20, chroma strength 0,0" in err
            assert found["block"] == 8 and found["origin"] == [3, 5] and found["chroma_origin"] is None and found["peaks"][0] == [[5, 13], [3, 11]]
            explicit = net3.upscale_video(v, deblock_block=8, deblock_origin=(3, 5), deblock_chroma_origin=(0, 0), deblock_chroma_strength=(0, 0), **fmt, **KW)
            assert torch.equal(want, explicit) and not torch.equal(want, net3.upscale_video(v, **fmt))
        else:
            assert "--deblock-grid auto: no grid found: --deblock none" in err and "--deblock strong" not in err
            assert found["block"] is None and torch.equal(want, net3.upscale_video(v, **fmt))
