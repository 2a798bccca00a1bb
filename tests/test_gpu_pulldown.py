"""GPU checks of the pulldown removal: savsr_video_field_scores_u8 / _u16 and savsr_video_weave against the numpy specification bit for
bit (row counts with no, one and many scored rows, row bytes across the 16-byte width and the workgroup's edge, unaligned pointers,
ranges with context, planes in place, the largest lane sums), the entries' refusals, remove_pulldown against the specification for every
frame kind, the property of upscale_video(pulldown=...) (bit for bit the call on the recovered film), what the feature is for (telecined
film upscales to what the film upscales to), VideoUpscaler(pulldown=...) under any chunking, the CLI."""
import io
import os

import numpy as np
import pytest
import torch

import savsr_amd
from savsr_amd import pulldown as pd
from savsr_amd import y4m, yuv
from savsr_amd.deinterlace import FIELD_ORDERS
from savsr_amd.utils import synth
from tests.pulldown_cases import noise_mats, packed_film, planar_film
from tests.video_cases import WEIGHT_SEED

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POISON = 0xA5
ROWS = (2, 3, 4, 5, 33)                           # 2: no scored row; 3: one, for one order only
ROW_BYTES = (1, 15, 16, 17, 256, 272, 319)        # the 16-byte width below / at / above, a full and a partial row of chunks, an odd width


def _lib():
    from savsr_amd import _lib as L
    return L.load()


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


def _upload(mats, depth, off, before, after):
    """The matrices [N, R, C] as the plane `before` bytes into frames of before + plane + after bytes, the first frame `off` bytes past a
    256-byte aligned allocation: (the device buffer, frame bytes, plane bytes)."""
    mats = np.ascontiguousarray(mats)
    n = mats.shape[0]
    plane = mats.astype("<u2").view(np.uint8).reshape(n, -1) if depth > 8 else mats.astype(np.uint8).reshape(n, -1)
    fb = before + plane.shape[1] + after
    host = np.full((n, fb), 0x3C, np.uint8)
    host[:, before:before + plane.shape[1]] = plane
    src = torch.empty(n * fb + off + 64, dtype=torch.uint8, device=DEV)
    assert src.data_ptr() % 256 == 0
    src[off:off + n * fb].copy_(torch.from_numpy(host).reshape(-1))
    return src, fb, plane.shape[1]


def _scores(mats, order, depth=8, rng=None, off=0, before=0, after=0):
    """One score entry of the C ABI on source frames [rng) (default: all) of the matrices; the scores lie between guard cells."""
    n, r, c = mats.shape
    lo, hi = rng or (0, n)
    src, fb, _ = _upload(mats, depth, off, before, after)
    out = torch.full((2 * (hi - lo) + 2,), -7, dtype=torch.int64, device=DEV)
    lib, st = _lib(), torch.cuda.current_stream().cuda_stream
    if depth > 8:
        rc = lib.savsr_video_field_scores_u16(src.data_ptr() + off, n, fb, before, r, c, depth, FIELD_ORDERS.index(order), lo, hi, out.data_ptr() + 8, st)
    else:
        rc = lib.savsr_video_field_scores_u8(src.data_ptr() + off, n, fb, before, r, c, FIELD_ORDERS.index(order), lo, hi, out.data_ptr() + 8, st)
    assert rc == 0, lib.savsr_last_error()
    got = out.cpu().numpy()
    assert got[0] == -7 and got[-1] == -7
    return got[1:-1].reshape(hi - lo, 2)


def _check_scores(mats, order, depth=8, **kw):
    lo, hi = kw.get("rng") or (0, mats.shape[0])
    got, want = _scores(mats, order, depth, **kw), pd.field_scores(mats, order, depth)[lo:hi]
    assert np.array_equal(got, want), (mats.shape, order, depth, kw, got.tolist(), want.tolist())


def _weave(mats, order, delta, rng=None, off=0, before=0, after=0, depth=8):
    """savsr_video_weave on source frames [rng) of the matrices, delta per output frame; the output frames have the input's layout, are
    poisoned first and are followed by guard bytes: nothing outside the planes is written."""
    n, r, c = mats.shape
    lo, hi = rng or (0, n)
    src, fb, pb = _upload(mats, depth, off, before, after)
    no = hi - lo
    dst = torch.full((no * fb + off + 64,), POISON, dtype=torch.uint8, device=DEV)
    table = torch.tensor(list(delta), dtype=torch.int32, device=DEV)
    lib, st = _lib(), torch.cuda.current_stream().cuda_stream
    rc = lib.savsr_video_weave(src.data_ptr() + off, n, fb, before, r, pb // r, FIELD_ORDERS.index(order), lo, hi, table.data_ptr(), dst.data_ptr() + off,
                               fb, before, st)
    assert rc == 0, lib.savsr_last_error()
    got = dst.cpu().numpy()
    assert (got[:off] == POISON).all() and (got[off + no * fb:] == POISON).all()
    got = got[off:off + no * fb].reshape(no, fb)
    assert (got[:, :before] == POISON).all() and (got[:, before + pb:] == POISON).all()
    got = got[:, before:before + pb]
    return np.ascontiguousarray(got).view("<u2").reshape(no, r, c) if depth > 8 else got.reshape(no, r, c)


def _check_weave(mats, order, delta, depth=8, **kw):
    lo, hi = kw.get("rng") or (0, mats.shape[0])
    want = pd.weave_matrix(mats, order, delta)[lo:hi]
    got = _weave(mats, order, delta[lo:hi], depth=depth, **kw)
    assert np.array_equal(got, want), (mats.shape, order, delta, depth, kw, np.argwhere(got != want)[:4])


# ---------------------------------------------------------------------------------------------------------------------- the score kernels
@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_field_scores_u8_equal_the_spec(order):
    """Every row count with every row length and frame count.  A row of a multiple of 16 bytes from an aligned pointer takes the vector
    form; the other lengths, and every length one byte off, take the one-sample form."""
    for r in ROWS:
        for rb in ROW_BYTES:
            v = noise_mats(6, r, rb, 255, seed=r * rb).astype(np.uint8)
            for n in (1, 2, 6):
                _check_scores(v[:n], order)
            _check_scores(v[:2], order, off=1)
    assert not _scores(noise_mats(2, 2, 16).astype(np.uint8), order).any()           # no scored row: the entry's zeros
    three = _scores(noise_mats(2, 3, 16).astype(np.uint8), order)
    assert bool(three.any()) == (order == "tff")                                     # y = 1 is the second field of tff alone


@pytest.mark.parametrize("depth", [10, 12])
@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_field_scores_u16_equal_the_spec(order, depth):
    """The same row lengths as 16-bit samples (8 of them are the 16-byte width), with samples above 2^d - 1 among them; two bytes off
    takes the one-sample form."""
    for r in ROWS:
        for c in (1, 7, 8, 9, 128, 136, 159):
            v = noise_mats(3, r, c, (1 << depth) - 1, seed=r + c).astype(np.uint16)
            v[:, 1::2, ::5] = 60000
            v[1, :, 1::3] = 1 << depth
            _check_scores(v, order, depth)
            _check_scores(v[:2], order, depth, off=2)


def test_field_scores_of_ranges_with_context():
    """from > 0 reads frame from - 1; from = 0 clamps; the plane may lie anywhere in its frame."""
    v = noise_mats(4, 9, 48, 255, seed=8).astype(np.uint8)
    w = noise_mats(4, 9, 24, 4095, seed=9).astype(np.uint16)
    for rng in ((0, 1), (1, 2), (1, 4), (3, 4), (0, 4), (2, 2)):
        for order in FIELD_ORDERS:
            for before, after in ((0, 0), (16, 32), (5, 3)):
                _check_scores(v, order, rng=rng, before=before, after=after)
            _check_scores(v, order, rng=rng, off=1)
            _check_scores(w, order, 12, rng=rng, before=16, after=6)
    # the range without its context is another video: frame 1 alone is its own predecessor
    assert not np.array_equal(_scores(v[1:2], "tff"), pd.field_scores(v, "tff")[1:2])


def test_field_scores_of_the_largest_lane_sums():
    """2 frames of 2048 x 64 bytes, 0 / 255 alternating by row parity: every scored sample adds 2 x 255, the most a sample can; the 32-bit
    lane and workgroup partials do not overflow and the 64-bit cells hold the sums."""
    tall = np.zeros((2, 2048, 64), np.uint8)
    tall[:, 1::2] = 255
    for order, rows in (("tff", 1023), ("bff", 1023)):
        want = pd.field_scores(tall, order)
        assert want.tolist() == [[rows * 64 * 510] * 2] * 2
        _check_scores(tall, order)
        _check_scores(tall, order, off=1)


def test_public_field_scores_of_every_frame_kind():
    rng = np.random.RandomState(10)
    for c in (1, 3):
        v = rng.randint(0, 256, size=(3, 9, 16, c), dtype=np.uint8)
        for order in FIELD_ORDERS:
            got = savsr_amd.field_scores(torch.from_numpy(v), order)
            assert got.device.type == "cuda" and got.dtype == torch.int64 and got.shape == (3, 2)
            assert np.array_equal(got.cpu().numpy(), pd.frame_scores(v, order))
    on_dev = torch.from_numpy(v).to(DEV)
    assert np.array_equal(savsr_amd.field_scores(on_dev, "bff").cpu().numpy(), pd.frame_scores(v, "bff"))
    for fmt, layout in (("i420", "420"), ("i444", "444")):
        for depth in (8, 10, 12):
            for h, w in ((9, 14), (16, 32)):
                fb = yuv.frame_bytes(h, w, depth, layout)
                if depth == 8:
                    frames = rng.randint(0, 256, size=(3, fb), dtype=np.uint8)
                else:
                    words = rng.randint(0, 1 << depth, size=(3, fb // 2))
                    words[:, ::7] = 50000                                            # above 2^d - 1: read as 2^d - 1
                    frames = words.astype("<u2").view(np.uint8).reshape(3, fb)
                got = savsr_amd.field_scores(torch.from_numpy(frames), "tff", fmt, (h, w), depth)
                assert np.array_equal(got.cpu().numpy(), pd.frame_scores(frames, "tff", fmt, (h, w), depth)), (fmt, depth, h, w)


# ---------------------------------------------------------------------------------------------------------------------- the weave kernel
@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_weave_equals_the_spec(order):
    """The score tests' row counts (and one row) and row lengths; delta all 0, all -1 (frame 0's clamps) and mixed; one byte off takes
    the byte form."""
    for r in (1,) + ROWS:
        for rb in ROW_BYTES:
            v = noise_mats(4, r, rb, 255, seed=r + rb).astype(np.uint8)
            for delta in ([0, 0, 0, 0], [-1, -1, -1, -1], [-1, 0, -1, 0]):
                _check_weave(v, order, delta)
            _check_weave(v, order, [0, -1, -1, 0], off=1)
    v = noise_mats(4, 9, 48, 255, seed=3).astype(np.uint8)
    for rng in ((1, 2), (0, 1), (1, 4), (3, 4)):                                     # a range with its context: n + delta is a resident frame
        for off in (0, 1):
            _check_weave(v, order, [-1, -1, 0, -1], rng=rng, off=off, before=16, after=16)


def test_weave_clamps_a_wrong_table_into_the_resident_frames():
    """The entry cannot see the device table: values outside -1 | 0 read a wrong frame, never outside the buffer."""
    v = noise_mats(3, 5, 16, 255, seed=4).astype(np.uint8)
    got = _weave(v, "tff", [-100, 100, 1])
    for n, m in enumerate((0, 2, 2)):
        assert np.array_equal(got[n, 0::2], v[n, 0::2]) and np.array_equal(got[n, 1::2], v[m, 1::2])


@pytest.mark.parametrize("depth", [8, 10])
def test_weave_the_planes_of_i420_frames_in_place(depth):
    """One call per plane through the plane offsets and the frame strides: 16 x 32, whose chroma planes of 8 x 16 have 16-byte rows at
    8 bits; 5 x 7, whose planes (chroma 3 x 4) are aligned nowhere."""
    for h, w in ((16, 32), (5, 7)):
        fb = yuv.frame_bytes(h, w, depth)
        rng = np.random.RandomState(h + depth)
        frames = rng.randint(0, 256, size=(4, fb), dtype=np.uint8)
        s = 1 if depth == 8 else 2
        before = 0
        for p in yuv.split_planes(frames, h, w, depth):
            size = p.shape[1] * p.shape[2] * s
            for delta in ([0, 0, 0, 0], [-1, -1, -1, -1], [0, -1, 0, -1]):
                _check_weave(p, "tff", delta, depth, before=before, after=fb - before - size)
            _check_weave(p, "bff", [-1, 0, -1, -1], depth, before=before, after=fb - before - size)
            before += size


def test_entries_refuse_bad_arguments():
    lib = _lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    out = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    table = torch.zeros(8, dtype=torch.int32, device=DEV)
    p, o, d = buf.data_ptr(), out.data_ptr(), table.data_ptr()
    s8, s16, wv = lib.savsr_video_field_scores_u8, lib.savsr_video_field_scores_u16, lib.savsr_video_weave
    bad = [
        # (frames, n_frames, frame_bytes, plane_offset, rows, row_bytes, order, from, to, out)
        (s8, (0, 2, 64, 0, 8, 8, 0, 0, 2, o), "null pointer"),
        (s8, (p, 2, 64, 0, 8, 8, 0, 0, 2, 0), "null pointer"),
        (s8, (p, 0, 64, 0, 8, 8, 0, 0, 0, o), "n_frames >= 1"),
        (s8, (p, 2, 64, 0, 0, 8, 0, 0, 2, o), "rows >= 1"),
        (s8, (p, 2, 64, 0, 8, 0, 0, 0, 2, o), "at least one sample"),
        (s8, (p, 2, 64, 0, 8, 8, 2, 0, 2, o), "order 0 (tff) or 1 (bff)"),
        (s8, (p, 2, 64, 0, 8, 8, -1, 0, 2, o), "order 0 (tff) or 1 (bff)"),
        (s8, (p, 2, 64, 0, 8, 8, 0, -1, 2, o), "0 <= from <= to <= n_frames"),
        (s8, (p, 2, 64, 0, 8, 8, 0, 0, 3, o), "0 <= from <= to <= n_frames"),
        (s8, (p, 2, 64, 0, 8, 8, 0, 2, 1, o), "0 <= from <= to <= n_frames"),
        (s8, (p, 2, 63, 0, 8, 8, 0, 0, 2, o), "frame_bytes smaller"),
        (s8, (p, 2, 64, 1, 8, 8, 0, 0, 2, o), "frame_bytes smaller"),
        (s8, (p, 2, 64, -1, 8, 8, 0, 0, 2, o), "plane offsets >= 0"),
        (s8, (p, 2, 64, 0, 8, 8, 0, 0, 2, o + 4), "8-byte aligned"),
        # (frames, n_frames, frame_bytes, plane_offset, rows, cols, depth, order, from, to, out)
        (s16, (p, 2, 128, 0, 8, 8, 8, 0, 0, 2, o), "depth 10 or 12"),
        (s16, (p, 2, 128, 0, 8, 8, 14, 0, 0, 2, o), "depth 10 or 12"),
        (s16, (p + 1, 2, 128, 0, 8, 8, 10, 0, 0, 2, o), "2-byte aligned"),
        (s16, (p, 2, 129, 0, 8, 8, 10, 0, 0, 2, o), "2-byte aligned"),
        (s16, (p, 2, 130, 1, 8, 8, 10, 0, 0, 2, o), "2-byte aligned"),
        (s16, (p, 2, 127, 0, 8, 8, 10, 0, 0, 2, o), "frame_bytes smaller"),
        (s16, (p, 2, 128, 0, 0, 8, 10, 0, 0, 2, o), "rows >= 1"),
        (s16, (0, 2, 128, 0, 8, 8, 10, 0, 0, 2, o), "null pointer"),
        (s16, (p, 2, 128, 0, 8, 8, 10, 0, 0, 2, 0), "null pointer"),
        (s16, (p, 2, 128, 0, 8, 8, 10, 3, 0, 2, o), "order 0 (tff) or 1 (bff)"),
        # (frames, n_frames, frame_bytes, plane_offset, rows, row_bytes, order, from, to, delta, out, out_frame_bytes, out_plane_offset)
        (wv, (0, 2, 64, 0, 8, 8, 0, 0, 2, d, o, 64, 0), "null pointer"),
        (wv, (p, 2, 64, 0, 8, 8, 0, 0, 2, 0, o, 64, 0), "null pointer"),
        (wv, (p, 2, 64, 0, 8, 8, 0, 0, 2, d, 0, 64, 0), "null pointer"),
        (wv, (p, 0, 64, 0, 8, 8, 0, 0, 0, d, o, 64, 0), "n_frames >= 1"),
        (wv, (p, 2, 64, 0, 0, 8, 0, 0, 2, d, o, 64, 0), "rows >= 1"),
        (wv, (p, 2, 64, 0, 8, 0, 0, 0, 2, d, o, 64, 0), "at least one sample"),
        (wv, (p, 2, 64, 0, 8, 8, 2, 0, 2, d, o, 64, 0), "order 0 (tff) or 1 (bff)"),
        (wv, (p, 2, 64, 0, 8, 8, 0, -1, 2, d, o, 64, 0), "0 <= from <= to <= n_frames"),
        (wv, (p, 2, 64, 0, 8, 8, 0, 0, 3, d, o, 64, 0), "0 <= from <= to <= n_frames"),
        (wv, (p, 2, 63, 0, 8, 8, 0, 0, 2, d, o, 64, 0), "frame_bytes smaller"),
        (wv, (p, 2, 64, 0, 8, 8, 0, 0, 2, d, o, 63, 0), "out_frame_bytes smaller"),
        (wv, (p, 2, 64, 0, 8, 8, 0, 0, 2, d, o, 64, 1), "out_frame_bytes smaller"),
        (wv, (p, 2, 64, 0, 8, 8, 0, 0, 2, d, o, 64, -1), "plane offsets >= 0"),
        (wv, (p, 2, 64, -1, 8, 8, 0, 0, 2, d, o, 64, 0), "plane offsets >= 0"),
        (wv, (p, 2, 64, 0, 8, 8, 0, 0, 2, d + 2, o, 64, 0), "delta must be 4-byte aligned"),
    ]
    out.fill_(POISON)
    torch.cuda.synchronize()
    for fn, args, words in bad:
        assert fn(*args, None) == -1, (fn.__name__, args)
        msg = lib.savsr_last_error().decode()
        assert words in msg and fn.__name__[len("savsr_"):] in msg, (fn.__name__, args, msg)
    torch.cuda.synchronize()
    assert bool((out == POISON).all())                                               # refused before the device is touched (not even the memset)
    for fn, args in ((s8, (p, 2, 64, 0, 8, 8, 0, 1, 1, o)), (wv, (p, 2, 64, 0, 8, 8, 0, 2, 2, d, o, 64, 0))):          # an empty range: nothing is done
        assert fn(*args, None) == 0
    torch.cuda.synchronize()
    assert bool((out == POISON).all())


# ---------------------------------------------------------------------------------------------------------------------- remove_pulldown
H, W = 16, 20
M = 8                                             # film frames: 10 video frames, two full cycles


def _video(kind="rgb", depth=8, seed=5, n=10):
    """Noise video: the kernels and the calls are exact whatever the data, and noise exercises both candidates."""
    rng = np.random.RandomState(seed)
    if kind == "rgb":
        return rng.randint(0, 256, size=(n, H, W, 3), dtype=np.uint8)
    fb = yuv.frame_bytes(H, W, depth, kind)
    if depth == 8:
        return rng.randint(0, 256, size=(n, fb), dtype=np.uint8)
    return rng.randint(0, 1 << depth, size=(n, fb // 2)).astype("<u2").view(np.uint8).reshape(n, fb)


def _same_info(got, want):
    assert np.array_equal(got["scores"], want["scores"]) and got["matches"] == want["matches"]
    assert np.array_equal(got["sad"], want["sad"]) and got["kept"] == want["kept"]


def test_remove_pulldown_equals_the_spec_for_every_frame_kind():
    cases = [("rgb", None, 8, _video()), ("rgb", None, 8, _video()[..., :1]),
             ("rgb", None, 8, pd.telecine(packed_film("bar", M, H, W), "tff")), ("rgb", None, 8, pd.telecine(packed_film("gradient", M, 9, 33), "bff", 1))]
    for fmt, layout, depth in (("i420", "420", 8), ("i420", "420", 10), ("i422", "422", 8), ("i444", "444", 12), ("y400", "400", 10)):
        cases.append((fmt, (H, W), depth, _video(layout, depth, seed=6 + depth)))
        cases.append((fmt, (H, W), depth, pd.telecine(planar_film("gradient", M, H, W, depth, layout), "tff", 0, fmt, (H, W), depth)))
    for fmt, size, depth, v in cases:
        for order in FIELD_ORDERS:
            want, winfo = pd.remove_pulldown_frames(v, order, fmt, size, depth)
            got, info = savsr_amd.remove_pulldown(torch.from_numpy(v), order, fmt, size, depth, return_info=True)
            assert got.device.type == "cuda" and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (fmt, depth, order)
            _same_info(info, winfo)
    v = _video(seed=7, n=9)
    for cycle in (2, 4, 9):
        want, winfo = pd.remove_pulldown_frames(v, "tff", cycle=cycle)
        got, info = savsr_amd.remove_pulldown(torch.from_numpy(v).to(DEV), "tff", cycle=cycle, return_info=True)
        assert np.array_equal(got.cpu().numpy(), want) and want.shape[0] == 9 - 9 // cycle
        _same_info(info, winfo)
    one = savsr_amd.remove_pulldown(torch.from_numpy(v[:1]), "bff")                  # one frame: its own predecessor, no pair, kept
    assert np.array_equal(one.cpu().numpy(), v[:1])


# ---------------------------------------------------------------------------------------------------------------------- the property
def _property(net, frames: np.ndarray, kw, more, out, scales=(2,), orders=FIELD_ORDERS, cycle=5):
    """upscale_video(v, pulldown=o) is upscale_video on the recovered film, the spec's and the GPU's (which are equal)."""
    fmt, size, depth = kw.get("pixel_format", "rgb"), kw.get("size"), kw.get("depth", 8)
    extra = {} if cycle == 5 else dict(pulldown_cycle=cycle)
    for order in orders:
        film = pd.remove_pulldown_frames(frames, order, fmt, size, depth, cycle)[0]
        on_gpu = savsr_amd.remove_pulldown(torch.from_numpy(frames), order, fmt, size, depth, cycle)
        assert np.array_equal(on_gpu.cpu().numpy(), film)
        for scale in scales:
            want = net.upscale_video(torch.from_numpy(film), scale=scale, out=out, **kw, **more)
            got = net.upscale_video(torch.from_numpy(frames), scale=scale, out=out, pulldown=order, **extra, **kw, **more)
            n = frames.shape[0]
            assert got.shape[0] == n - n // cycle and got.shape == want.shape and torch.equal(got, want), (out, order, scale)


def test_property_uint8(net3):
    _property(net3, _video(), {}, {}, "uint8", scales=(2, (2.5, 3.0)))
    _property(net3, _video(seed=8, n=9), {}, {}, "uint8", orders=("tff",), cycle=3)


def test_property_i420(net3):
    _property(net3, _video("420", 8), dict(pixel_format="i420", size=(H, W)), {}, "i420")


def test_property_i420_10_bits(net3):
    _property(net3, _video("420", 10), dict(pixel_format="i420", size=(H, W), depth=10), dict(out_depth=10), "i420", orders=("bff",))


def test_property_luma_only_y400(net1):
    _property(net1, _video(yuv.MONO, 8), dict(pixel_format="y400", size=(H, W)), {}, "y400", orders=("tff",))


def test_property_with_cuts(net3):
    """Explicit cuts index the film frames; "auto" scores them."""
    v = _video(seed=9)
    _property(net3, v, {}, dict(cuts=[4]), "uint8", orders=("tff",))
    _property(net3, v, {}, dict(cuts="auto"), "uint8", orders=("bff",))
    with pytest.raises(ValueError, match="cut 8"):                                   # 0 < k < N - N // 5 = 8
        net3.upscale_video(torch.from_numpy(v), scale=2, pulldown="tff", cuts=[8])


def test_property_with_crop_auto(net3):
    """Pulldown removal comes before the crop: the detector reads the film frames."""
    rng = np.random.RandomState(10)
    v = rng.randint(12, 25, size=(10, H, W, 3)).astype(np.uint8)
    v[:, 4:12, 2:18] = rng.randint(60, 256, size=(10, 8, 16, 3))
    film = pd.remove_pulldown_frames(v, "tff")[0]
    assert savsr_amd.detect_active_area(torch.from_numpy(film)) == (4, 2, 8, 16)
    want = net3.upscale_video(torch.from_numpy(film), scale=2, out="uint8", crop=(4, 2, 8, 16))
    assert torch.equal(net3.upscale_video(torch.from_numpy(v), scale=2, out="uint8", pulldown="tff", crop="auto"), want)
    _property(net3, v, {}, dict(crop="auto", bars="drop"), "uint8", orders=("bff",))


def test_property_with_the_self_ensemble(net3):
    net3.set_self_ensemble(True)
    try:
        _property(net3, _video(seed=11), {}, {}, "uint8", orders=("tff",))
    finally:
        net3.set_self_ensemble(False)


def test_property_in_fp16(net3):
    net3.set_precision("fp16")
    try:
        _property(net3, _video("420", 8, 12), dict(pixel_format="i420", size=(H, W)), {}, "i420", scales=((2.5, 3.0),), orders=("bff",))
    finally:
        net3.set_precision("fp32")


@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_telecined_film_upscales_to_what_the_film_upscales_to(net3, order):
    """What the feature is for: upscale_video(telecine(film), pulldown=o) == upscale_video(film), bit for bit, for a phase-0 film."""
    film = packed_film("bar", M, H, W)
    video = pd.telecine(film, order)
    assert video.shape[0] == 10
    want = net3.upscale_video(torch.from_numpy(film), scale=2, out="uint8")
    assert torch.equal(net3.upscale_video(torch.from_numpy(video), scale=2, out="uint8", pulldown=order), want)
    planar = planar_film("gradient", M, H, W)
    kw = dict(out="i420", pixel_format="i420", size=(H, W))
    want = net3.upscale_video(torch.from_numpy(planar), scale=2, **kw)
    assert torch.equal(net3.upscale_video(torch.from_numpy(pd.telecine(planar, order, 0, "i420", (H, W))), scale=2, pulldown=order, **kw), want)


def test_pulldown_none_is_the_call_without_the_argument(net3):
    v = torch.from_numpy(_video(seed=13, n=8))
    assert torch.equal(net3.upscale_video(v, scale=2, out="uint8", pulldown=None), net3.upscale_video(v, scale=2, out="uint8"))
    with pytest.raises(ValueError, match="float frames have no integer samples"):
        net3.upscale_video(v.to(DEV).float().permute(0, 3, 1, 2).contiguous() / 255, scale=2, pulldown="tff")


# ---------------------------------------------------------------------------------------------------------------------- streaming
@pytest.mark.parametrize("chunk", [1, 2, 3, 7])
def test_video_upscaler_with_pulldown_any_chunking_is_bitwise(net3, chunk):
    from savsr_amd import VideoUpscaler
    n = 13                                                                            # two full cycles and a partial one of three
    u8 = torch.from_numpy(_video(seed=14, n=n))
    whole, winfo = savsr_amd.remove_pulldown(u8, "tff", return_info=True)
    whole8 = net3.upscale_video(u8, scale=2, out="uint8", pulldown="tff")
    up = VideoUpscaler(net3, 2, out="uint8", pulldown="tff")
    parts = []
    for a in range(0, n, chunk):
        parts.append(up.push(u8[a:a + chunk]))
        rem = up._split
        assert 1 <= rem.held <= 5 + 1 and (rem._pend is None or rem._pend.shape[0] <= 4)
        for t in (rem._ctx, rem._last, rem._pend):                                   # copies of their own: the chunk's storage is released
            assert t is None or t.untyped_storage().nbytes() == t.numel() * t.element_size()
    parts.append(up.finish())
    assert all(p.shape[1:] == whole8.shape[1:] for p in parts)                       # the empty returns have the output's size too
    assert torch.equal(torch.cat(parts, 0), whole8) and up._buf is None and up._split.held == 0
    assert up.pulldown_info == {"matches": winfo["matches"], "kept": winfo["kept"]} and whole.shape[0] == 11
    yv = torch.from_numpy(_video("420", 10, 15, n))
    kw = dict(out="i420", pixel_format="i420", size=(H, W), depth=10, out_depth=10)
    whole = net3.upscale_video(yv, scale=2, pulldown="bff", pulldown_cycle=4, cuts="auto", crop=(2, 4, 11, 13), **kw)
    up = VideoUpscaler(net3, 2, pulldown="bff", pulldown_cycle=4, cuts="auto", crop=(2, 4, 11, 13), **kw)
    parts = [up.push(yv[a:a + chunk]) for a in range(0, n, chunk)] + [up.finish()]
    assert torch.equal(torch.cat(parts, 0), whole), chunk
    assert VideoUpscaler(net3, 2).pulldown_info is None


# ---------------------------------------------------------------------------------------------------------------------- the CLI
def test_cli_y4m_pulldown(net3, tmp_path, capsys):
    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    frames = pd.telecine(planar_film("bar", M, H, W), "tff", 0, "i420", (H, W))
    assert frames.shape[0] == 10
    f = io.BytesIO()
    y4m.Y4MWriter(f, W, H, (30000, 1001), "t", (1, 1)).write(frames)
    src, ckpt = tmp_path / "lr.y4m", tmp_path / "net.pth"
    src.write_bytes(f.getvalue())
    sio.save_network(net3, str(ckpt))
    kw = dict(out="i420", pixel_format="i420", size=(H, W))
    base = ["-i", str(src), "--scale", "2", "--checkpoint", str(ckpt), "--chunk", "3"]

    def expect(sr, fps, tag):
        g = io.BytesIO()
        y4m.Y4MWriter(g, 2 * W, 2 * H, fps, tag, y4m.scaled_aspect((1, 1), (H, W), (2 * H, 2 * W))).write(sr.cpu().numpy())
        return g.getvalue()

    # --pulldown auto: It -> tff, the output is progressive at 4 / 5 of the rate and holds the 8 film frames
    dst = tmp_path / "sr24p.y4m"
    assert main(base + ["-o", str(dst), "--pulldown", "auto"]) == 0
    sr = net3.upscale_video(torch.from_numpy(frames), scale=2, pulldown="tff", **kw)
    want = expect(sr, (24000, 1001), "p")
    assert sr.shape[0] == 8 and dst.read_bytes() == want and b" F24000:1001 Ip " in want[:80]
    assert torch.equal(sr, net3.upscale_video(torch.from_numpy(planar_film("bar", M, H, W)), scale=2, **kw))          # the film's own frames
    cap = capsys.readouterr()
    assert "treated as progressive" not in cap.err
    assert "pulldown tff: 10 frames in, 8 out, 4 matched from their predecessor" in cap.out
    # an explicit order and cycle override the tag
    dst = tmp_path / "sr_bff.y4m"
    assert main(base + ["-o", str(dst), "--pulldown", "bff", "--pulldown-cycle", "4"]) == 0
    sr = net3.upscale_video(torch.from_numpy(frames), scale=2, pulldown="bff", pulldown_cycle=4, **kw)
    assert sr.shape[0] == 8 and dst.read_bytes() == expect(sr, (22500, 1001), "p")
    # a PNG-folder output holds the kept frames
    out_dir = tmp_path / "png"
    assert main(base + ["-o", str(out_dir), "--pulldown", "tff"]) == 0
    assert sorted(os.listdir(out_dir)) == [f"{k:08d}.png" for k in range(8)]
    # without the flag nothing changes: the woven frames as ever, the tag passed through, the note
    capsys.readouterr()
    dst = tmp_path / "sr_woven.y4m"
    assert main(base + ["-o", str(dst)]) == 0
    cap = capsys.readouterr()
    assert cap.err.count("treated as progressive") == 1 and "pulldown" not in cap.out
    want = expect(net3.upscale_video(torch.from_numpy(frames), scale=2, **kw), (30000, 1001), "t")
    assert dst.read_bytes() == want and b" F30000:1001 It " in want[:80]
    # Im (mixed) is refused by name
    f = io.BytesIO()
    y4m.Y4MWriter(f, W, H, (30000, 1001), "m", (1, 1)).write(frames)
    src.write_bytes(f.getvalue())
    with pytest.raises(SystemExit, match="Im"):
        main(base + ["-o", str(tmp_path / "x.y4m"), "--pulldown", "auto"])
