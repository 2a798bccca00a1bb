"""GPU checks of combed=: savsr_video_comb_windows_u8 / _u16 and savsr_video_deinterlace_masked_u8 / _u16 against the numpy specification
bit for bit (row counts around the cell, row bytes around the 16-byte chunk and the cell, several tiles each way, both pixel steps, every
depth, unaligned pointers, ranges with context, guard cells, the largest counts, noise), the entries' refusals, remove_pulldown(combed=)
against the specification for every frame kind, the property of upscale_video(combed=...), VideoUpscaler under any chunking with the bound
on the frames it holds, the CLI."""
import io

import numpy as np
import pytest
import torch

import savsr_amd
from savsr_amd import pulldown as pd
from savsr_amd import y4m
from savsr_amd.deinterlace import DEINTERLACERS, FIELD_ORDERS, bwdif_matrix, deinterlace_matrix
from savsr_amd.utils import synth
from tests import combed_cases as cc
from tests.pulldown_cases import noise_mats, packed_film
from tests.video_cases import WEIGHT_SEED

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POISON = 0xA5
ROWS = (2, 3, 4, 5, 9, 17, 33)
ROW_BYTES = (1, 7, 8, 9, 15, 16, 17, 33, 272, 319)


def _lib():
    from savsr_amd import _lib as L
    return L.load()


@pytest.fixture(scope="module")
def net3():
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=WEIGHT_SEED), strict=True)
    return net.to(DEV).eval()


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


def _comb(mats, order, step=1, depth=8, threshold=9, rng=None, off=0, before=0, after=0):
    """One comb entry of the C ABI on frames [rng) (default: all) of the matrices; the counts lie between guard cells."""
    n, r, c = mats.shape
    lo, hi = rng or (0, n)
    src, fb, _ = _upload(mats, depth, off, before, after)
    out = torch.full((2 * (hi - lo) + 2,), -7, dtype=torch.int64, device=DEV)
    lib, st = _lib(), torch.cuda.current_stream().cuda_stream
    if depth > 8:
        rc = lib.savsr_video_comb_windows_u16(src.data_ptr() + off, n, fb, before, r, c, depth, FIELD_ORDERS.index(order), lo, hi, threshold,
                                              out.data_ptr() + 8, st)
    else:
        rc = lib.savsr_video_comb_windows_u8(src.data_ptr() + off, n, fb, before, r, c, step, FIELD_ORDERS.index(order), lo, hi, threshold,
                                             out.data_ptr() + 8, st)
    assert rc == 0, lib.savsr_last_error()
    got = out.cpu().numpy()
    assert got[0] == -7 and got[-1] == -7
    return got[1:-1].reshape(hi - lo, 2)


def _check_comb(mats, order, step=1, depth=8, threshold=9, **kw):
    lo, hi = kw.get("rng") or (0, mats.shape[0])
    got, want = _comb(mats, order, step, depth, threshold, **kw), pd.comb_windows(mats, order, step, threshold, depth)[lo:hi]
    assert np.array_equal(got, want), (mats.shape, order, step, depth, threshold, kw, got.tolist(), want.tolist())


def _soft(n, r, c, top, seed):
    """Noise of a small spread around a level per frame: some samples combed, some not, at the default threshold."""
    rng = np.random.RandomState(seed)
    return (rng.randint(0, top + 1, size=(n, 1, 1)) // 2 + rng.randint(0, top + 1, size=(n, r, c)) // 8)


# ---------------------------------------------------------------------------------------------------------------------- the comb kernels
@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_comb_windows_u8_equal_the_spec(order, step):
    """Every row count with every row length.  A row of a multiple of 16 bytes from an aligned pointer takes the vector form; the other
    lengths, and every length one byte off, take the one-sample form."""
    for r in ROWS:
        for rb in ROW_BYTES:
            v = _soft(3, r, rb, 255, r * rb).astype(np.uint8)
            _check_comb(v, order, step)
            _check_comb(v[:2], order, step, off=1)
            _check_comb(noise_mats(2, r, rb, 255, seed=r + rb).astype(np.uint8), order, step, threshold=40)
    assert not _comb(noise_mats(2, 2, 16).astype(np.uint8), order, step).any()        # no scored row: the entry's zeros
    three = _comb(noise_mats(2, 3, 16).astype(np.uint8), order, step, threshold=0)
    assert bool(three.any()) == (order == "tff")                                      # y = 1 is the second field of tff alone


@pytest.mark.parametrize("depth", [10, 12])
@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_comb_windows_u16_equal_the_spec(order, depth):
    """The same row lengths as 16-bit samples (8 of them are the 16-byte width and one cell), with samples above 2^d - 1 among them; two
    bytes off takes the one-sample form."""
    for r in ROWS:
        for c in (1, 7, 8, 9, 15, 16, 17, 33, 136, 159):
            v = _soft(3, r, c, (1 << depth) - 1, r + c).astype(np.uint16)
            v[:, 1::2, ::5] = 60000
            v[1, :, 1::3] = 1 << depth
            _check_comb(v, order, 1, depth)
            _check_comb(v[:2], order, 1, depth, off=2)


def test_comb_windows_over_several_tiles():
    """A workgroup's tile is 64 rows x 512 bytes of window origins with a halo of one cell row and column: 145 rows are three tile rows
    (the last one a single clipped cell row), 1072 bytes three tile columns at step 1 and 528 / 24 = 22 cell columns = two tiles (21 and
    1) at step 3; windows across every tile boundary are summed from the halo, totals count no halo cell twice."""
    v = _soft(2, 145, 1072, 255, 5).astype(np.uint8)
    v[0, 60:76, 500:530] = np.where(np.arange(16)[:, None] % 2, 255, 0)               # a comb patch across a tile corner
    v[1, 120:145, 1040:1072] = np.where(np.arange(25)[:, None] % 2, 0, 255)
    for order in FIELD_ORDERS:
        for step in (1, 2, 3, 4):
            _check_comb(v, order, step)
            _check_comb(v[:, :, :1071], order, step)                                  # the one-sample form, by the row length
        _check_comb(v[:, :131, :528], order, 3, off=1)
        w = (v[:, :, :600].astype(np.uint16) << 2) | 3
        _check_comb(w, order, 1, 10)
        _check_comb(w[:, :, :599], order, 1, 10)


def test_comb_windows_of_ranges_with_context():
    """The measure of frame n reads frame n alone: a range gives the rows of the whole call; the plane may lie anywhere in its frame."""
    v = _soft(4, 19, 48, 255, 8).astype(np.uint8)
    w = _soft(4, 19, 24, 4095, 9).astype(np.uint16)
    for rng in ((0, 1), (1, 2), (1, 4), (3, 4), (0, 4), (2, 2)):
        for order in FIELD_ORDERS:
            for before, after in ((0, 0), (16, 32), (5, 3)):
                _check_comb(v, order, 3, rng=rng, before=before, after=after)
            _check_comb(v, order, rng=rng, off=1)
            _check_comb(w, order, 1, 12, rng=rng, before=16, after=6)


def test_comb_windows_of_the_all_combed_frame():
    """0 / 255 alternating by row parity: every scored sample is combed at every threshold below 255: the largest counts a window (128
    pixels) and a frame can have; threshold 255 (the measure is at most 510) flags nothing."""
    full = np.zeros((2, 145, 1072), np.uint8)
    full[:, 1::2] = 255
    for order, rows in (("tff", 72), ("bff", 71)):
        want = pd.comb_windows(full, order)
        assert want.tolist() == [[128, rows * 1072]] * 2
        _check_comb(full, order)
        _check_comb(full, order, off=1)
        _check_comb(full, order, 4, threshold=254)
        assert pd.comb_windows(full, order, 4).tolist() == [[512, rows * 1072]] * 2
        assert not _comb(full, order, threshold=255).any()


def test_public_comb_windows_of_every_frame_kind():
    from savsr_amd import yuv
    rng = np.random.RandomState(10)
    for c in (1, 3):
        v = (rng.randint(0, 256, size=(3, 17, 20, c)) // 6).astype(np.uint8)
        for order in FIELD_ORDERS:
            got = savsr_amd.comb_windows(torch.from_numpy(v), order)
            assert got.device.type == "cuda" and got.dtype == torch.int64 and got.shape == (3, 2)
            assert np.array_equal(got.cpu().numpy(), pd.frame_comb_windows(v, order)) and got.any()
    assert np.array_equal(savsr_amd.comb_windows(torch.from_numpy(v).to(DEV), "bff", threshold=3).cpu().numpy(), pd.frame_comb_windows(v, "bff", threshold=3))
    for fmt, layout in (("i420", "420"), ("i444", "444")):
        for depth in (8, 10, 12):
            for h, w in ((9, 14), (16, 32)):
                fb = yuv.frame_bytes(h, w, depth, layout)
                if depth == 8:
                    frames = (rng.randint(0, 256, size=(3, fb)) // 6).astype(np.uint8)
                else:
                    words = rng.randint(0, 1 << depth, size=(3, fb // 2)) // 6
                    words[:, ::7] = 50000                                             # above 2^d - 1: read as 2^d - 1
                    frames = words.astype("<u2").view(np.uint8).reshape(3, fb)
                got = savsr_amd.comb_windows(torch.from_numpy(frames), "tff", fmt, (h, w), depth)
                assert np.array_equal(got.cpu().numpy(), pd.frame_comb_windows(frames, "tff", fmt, (h, w), depth)), (fmt, depth, h, w)


# ---------------------------------------------------------------------------------------------------------------------- the masked deinterlacer
def _masked(mats, order, method, flags, step=1, depth=8, rng=None, off=0, before=0, after=0):
    """One masked entry of the C ABI on source frames [rng) of the matrices; the output frames have the input's layout, are poisoned
    first and are followed by guard bytes: nothing outside the planes is written."""
    n, r, c = mats.shape
    lo, hi = rng or (0, n)
    src, fb, pb = _upload(mats, depth, off, before, after)
    no = hi - lo
    dst = torch.full((no * fb + off + 64,), POISON, dtype=torch.uint8, device=DEV)
    table = torch.tensor(list(flags[lo:hi]), dtype=torch.int32, device=DEV)
    lib, st = _lib(), torch.cuda.current_stream().cuda_stream
    oid, mid = FIELD_ORDERS.index(order), DEINTERLACERS.index(method)
    if depth > 8:
        rc = lib.savsr_video_deinterlace_masked_u16(src.data_ptr() + off, n, fb, before, r, c, depth, oid, lo, hi, dst.data_ptr() + off, fb, before, mid,
                                                    table.data_ptr(), st)
    else:
        rc = lib.savsr_video_deinterlace_masked_u8(src.data_ptr() + off, n, fb, before, r, c, step, oid, lo, hi, dst.data_ptr() + off, fb, before, mid,
                                                   table.data_ptr(), st)
    assert rc == 0, lib.savsr_last_error()
    got = dst.cpu().numpy()
    assert (got[:off] == POISON).all() and (got[off + no * fb:] == POISON).all()
    got = got[off:off + no * fb].reshape(no, fb)
    assert (got[:, :before] == POISON).all() and (got[:, before + pb:] == POISON).all()
    got = got[:, before:before + pb]
    return np.ascontiguousarray(got).view("<u2").reshape(no, r, c) if depth > 8 else got.reshape(no, r, c)


_CLEAN = {}


def _clean(mats, order, method, step, depth):
    """The same-rate deinterlaced matrices (computed once per input: the reference is shared by the flag patterns)."""
    key = (id(mats), order, method, step, depth)
    if key not in _CLEAN:
        _CLEAN[key] = (mats, (bwdif_matrix(mats, order, depth)[0] if method == "bwdif" else deinterlace_matrix(mats, order, step, depth)[0])[0::2])
    return _CLEAN[key][1]


def _check_masked(mats, order, method, flags, step=1, depth=8, **kw):
    lo, hi = kw.get("rng") or (0, mats.shape[0])
    clean = _clean(mats, order, method, step, depth)
    want = np.where(np.asarray(flags, dtype=bool)[:, None, None], clean, mats)[lo:hi]
    got = _masked(mats, order, method, flags, step, depth, **kw)
    assert np.array_equal(got, want), (mats.shape, order, method, flags, step, depth, kw, np.argwhere(got != want)[:4])
    for k in range(lo, hi):                                                           # unflagged frames are byte copies, also of samples above 2^d - 1
        assert flags[k] or np.array_equal(got[k - lo], mats[k])


@pytest.mark.parametrize("method", DEINTERLACERS)
@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_deinterlace_masked_equals_the_spec(order, method):
    """Flags all 0, all 1 and alternating both ways (flagged frames at index 0 and N - 1: clamped neighbours); shapes with no inner row, no
    line row, both forms; one byte off takes the one-sample form."""
    for r, c in ((2, 1), (3, 1), (5, 7), (8, 16), (9, 33), (10, 32), (13, 48), (33, 272)):
        v = noise_mats(4, r, c, 255, seed=r + c).astype(np.uint8)
        w = noise_mats(4, r, c, 4500, seed=r * c).astype(np.uint16)
        for flags in ([0, 0, 0, 0], [1, 1, 1, 1], [1, 0, 1, 0], [0, 1, 0, 1]):
            _check_masked(v, order, method, flags)
            _check_masked(v, order, method, flags, off=1)
            _check_masked(w, order, method, flags, depth=12)
            _check_masked(w, order, method, flags, depth=10, off=2)
        if c % 3 == 0:
            _check_masked(v, order, method, [1, 0, 0, 1], step=3)


def test_deinterlace_masked_of_ranges_with_context():
    v = noise_mats(4, 13, 48, 255, seed=3).astype(np.uint8)
    for method in DEINTERLACERS:
        for rng in ((1, 2), (0, 1), (1, 4), (3, 4)):
            for off in (0, 1):
                _check_masked(v, "tff", method, [1, 1, 0, 1], step=3, rng=rng, off=off, before=16, after=16)
                _check_masked(v, "bff", method, [0, 1, 1, 0], rng=rng, off=off, before=5, after=3)
    # a flag that is any value but 0 is a set flag
    assert np.array_equal(_masked(v, "tff", "bwdif", [-1, 7, 0, 1 << 30]), _masked(v, "tff", "bwdif", [1, 1, 0, 1]))


def test_entries_refuse_bad_arguments():
    lib = _lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    out = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    table = torch.zeros(8, dtype=torch.int32, device=DEV)
    p, o, d = buf.data_ptr(), out.data_ptr(), table.data_ptr()
    c8, c16 = lib.savsr_video_comb_windows_u8, lib.savsr_video_comb_windows_u16
    m8, m16 = lib.savsr_video_deinterlace_masked_u8, lib.savsr_video_deinterlace_masked_u16
    bad = [
        # (frames, n_frames, frame_bytes, plane_offset, rows, row_bytes, step, order, from, to, threshold, out)
        (c8, (0, 2, 64, 0, 8, 8, 1, 0, 0, 2, 9, o), "null pointer"),
        (c8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 2, 9, 0), "null pointer"),
        (c8, (p, 0, 64, 0, 8, 8, 1, 0, 0, 0, 9, o), "n_frames >= 1"),
        (c8, (p, 2, 64, 0, 0, 8, 1, 0, 0, 2, 9, o), "rows >= 1"),
        (c8, (p, 2, 64, 0, 8, 0, 1, 0, 0, 2, 9, o), "at least one sample"),
        (c8, (p, 2, 64, 0, 8, 8, 0, 0, 0, 2, 9, o), "step 1 .. 4"),
        (c8, (p, 2, 64, 0, 8, 8, 5, 0, 0, 2, 9, o), "step 1 .. 4"),
        (c8, (p, 2, 64, 0, 8, 8, 1, 2, 0, 2, 9, o), "order 0 (tff) or 1 (bff)"),
        (c8, (p, 2, 64, 0, 8, 8, 1, 0, -1, 2, 9, o), "0 <= from <= to <= n_frames"),
        (c8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 3, 9, o), "0 <= from <= to <= n_frames"),
        (c8, (p, 2, 64, 0, 8, 8, 1, 0, 2, 1, 9, o), "0 <= from <= to <= n_frames"),
        (c8, (p, 2, 63, 0, 8, 8, 1, 0, 0, 2, 9, o), "frame_bytes smaller"),
        (c8, (p, 2, 64, -1, 8, 8, 1, 0, 0, 2, 9, o), "plane offsets >= 0"),
        (c8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 2, -1, o), "threshold 0 .. 255"),
        (c8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 2, 256, o), "threshold 0 .. 255"),
        (c8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 2, 9, o + 4), "8-byte aligned"),
        # (frames, n_frames, frame_bytes, plane_offset, rows, cols, depth, order, from, to, threshold, out)
        (c16, (p, 2, 128, 0, 8, 8, 8, 0, 0, 2, 9, o), "depth 10 or 12"),
        (c16, (p + 1, 2, 128, 0, 8, 8, 10, 0, 0, 2, 9, o), "2-byte aligned"),
        (c16, (p, 2, 129, 0, 8, 8, 10, 0, 0, 2, 9, o), "2-byte aligned"),
        (c16, (p, 2, 130, 1, 8, 8, 10, 0, 0, 2, 9, o), "2-byte aligned"),
        (c16, (p, 2, 127, 0, 8, 8, 10, 0, 0, 2, 9, o), "frame_bytes smaller"),
        (c16, (0, 2, 128, 0, 8, 8, 10, 0, 0, 2, 9, o), "null pointer"),
        (c16, (p, 2, 128, 0, 8, 8, 10, 0, 0, 2, 9, 0), "null pointer"),
        (c16, (p, 2, 128, 0, 8, 8, 12, 0, 0, 2, 300, o), "threshold 0 .. 255"),
        # (frames, n_frames, frame_bytes, plane_offset, rows, row_bytes, step, order, from, to, out, out_frame_bytes, out_plane_offset, method, flags)
        (m8, (0, 2, 64, 0, 8, 8, 1, 0, 0, 2, o, 64, 0, 0, d), "null pointer"),
        (m8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 2, 0, 64, 0, 0, d), "null pointer"),
        (m8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 2, o, 64, 0, 0, 0), "null pointer"),
        (m8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 2, o, 64, 0, 0, d + 2), "flags must be 4-byte aligned"),
        (m8, (p, 2, 64, 0, 1, 8, 1, 0, 0, 2, o, 64, 0, 0, d), "rows >= 2"),
        (m8, (p, 2, 64, 0, 8, 8, 0, 0, 0, 2, o, 64, 0, 0, d), "step 1 .. 4"),
        (m8, (p, 2, 64, 0, 8, 8, 3, 0, 0, 2, o, 64, 0, 0, d), "step 1 .. 4 and a divisor"),
        (m8, (p, 2, 64, 0, 8, 8, 1, 2, 0, 2, o, 64, 0, 0, d), "order 0 (tff) or 1 (bff)"),
        (m8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 3, o, 64, 0, 0, d), "0 <= from < to <= n_frames"),
        (m8, (p, 2, 64, 0, 8, 8, 1, 0, 1, 1, o, 64, 0, 0, d), "0 <= from < to <= n_frames"),
        (m8, (p, 2, 63, 0, 8, 8, 1, 0, 0, 2, o, 64, 0, 0, d), "frame_bytes smaller"),
        (m8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 2, o, 63, 0, 0, d), "out_frame_bytes smaller"),
        (m8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 2, o, 64, 0, 2, d), "method 0 (yadif) or 1 (bwdif)"),
        (m8, (p, 2, 64, 0, 8, 8, 1, 0, 0, 2, p + 64, 64, 0, 0, d), "overlap"),
        (m8, (p + 64, 2, 64, 0, 8, 8, 1, 0, 1, 2, p, 128, 0, 1, d), "overlap"),
        # (frames, n_frames, frame_bytes, plane_offset, rows, cols, depth, order, from, to, out, out_frame_bytes, out_plane_offset, method, flags)
        (m16, (p, 2, 128, 0, 8, 8, 8, 0, 0, 2, o, 128, 0, 0, d), "depth 10 or 12"),
        (m16, (p + 1, 2, 128, 0, 8, 8, 10, 0, 0, 2, o, 128, 0, 0, d), "2-byte aligned"),
        (m16, (p, 2, 129, 0, 8, 8, 10, 0, 0, 2, o, 128, 0, 0, d), "2-byte aligned"),
        (m16, (p, 2, 128, 0, 8, 8, 10, 0, 0, 2, o, 129, 0, 0, d), "2-byte aligned"),
        (m16, (p, 2, 128, 0, 8, 8, 10, 0, 0, 2, o, 128, 0, 0, 0), "null pointer"),
        (m16, (p, 2, 128, 0, 8, 8, 10, 0, 0, 2, o, 128, 0, -1, d), "method 0 (yadif) or 1 (bwdif)"),
        (m16, (p, 2, 128, 0, 8, 8, 12, 0, 0, 2, p + 254, 128, 0, 0, d), "overlap"),
    ]
    out.fill_(POISON)
    torch.cuda.synchronize()
    for fn, args, words in bad:
        assert fn(*args, None) == -1, (fn.__name__, args)
        msg = lib.savsr_last_error().decode()
        assert words in msg and fn.__name__[len("savsr_"):] in msg, (fn.__name__, args, msg)
    torch.cuda.synchronize()
    assert bool((out == POISON).all())                                                # refused before the device is touched (not even the memset)
    assert c8(p, 2, 64, 0, 8, 8, 1, 0, 1, 1, 9, o, None) == 0                          # an empty range: nothing is done
    torch.cuda.synchronize()
    assert bool((out == POISON).all())


def test_abi_surface():
    from savsr_amd import _lib as L
    import inspect
    lib = _lib()
    assert L.ABI_VERSION >= 49 and lib.savsr_abi_version() == L.ABI_VERSION
    for name in ("savsr_video_comb_windows_u8", "savsr_video_comb_windows_u16", "savsr_video_deinterlace_masked_u8", "savsr_video_deinterlace_masked_u16"):
        assert hasattr(lib, name), name
    for name in ("combed", "comb_threshold", "comb_pixels"):
        for fn in (savsr_amd.remove_pulldown, savsr_amd.SAVSR.upscale_video, savsr_amd.VideoUpscaler.__init__, savsr_amd.video.upscale_video):
            assert inspect.signature(fn).parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, (fn, name)


# ---------------------------------------------------------------------------------------------------------------------- remove_pulldown
H, W = 16, 16
KINDS = [("rgb", None, 8), ("i420", (H, W), 8), ("i422", (H, W), 10), ("y400", (H, W), 8)]


def _same_info(got, want):
    assert sorted(got) == sorted(want) == ["comb", "combed", "kept", "matches", "sad", "scores"]
    assert np.array_equal(got["scores"], want["scores"]) and got["matches"] == want["matches"]
    assert np.array_equal(got["sad"], want["sad"]) and got["kept"] == want["kept"]
    assert np.array_equal(got["comb"], want["comb"]) and got["comb"].dtype == np.int64 and got["combed"] == want["combed"]


@pytest.mark.parametrize("fmt,size,depth", KINDS)
def test_remove_pulldown_combed_equals_the_spec(fmt, size, depth):
    kw = {} if fmt == "rgb" else dict(pixel_format=fmt, size=size, depth=depth)
    cases = []
    for h, w in ((H, W), (33, 50)) if fmt == "rgb" else ((H, W),):
        if fmt != "rgb":
            kw["size"] = (h, w)
        video, insert = cc.hybrid("tff", h, w, fmt=fmt, depth=depth)
        cases.append((video, "tff", dict(kw), insert))
    video, insert = cc.hybrid("bff", 48, 64, fmt=fmt, depth=depth, parts=(4, 4, 8), phase=2)
    cases.append((video, "bff", dict(kw, size=(48, 64)) if fmt != "rgb" else {}, None))
    rng = np.random.RandomState(depth)
    noise = (video.astype(np.int64) + rng.randint(0, 4, size=video.shape)).clip(0, 255).astype(np.uint8) if depth == 8 else video
    cases.append((noise, "tff", cases[-1][2], None))                                  # (the wrong order: many frames flagged, both candidates exercised)
    for video, order, k, insert in cases:
        for method in DEINTERLACERS:
            want, winfo = pd.remove_pulldown_frames(video, order, combed=method, **k)
            got, info = savsr_amd.remove_pulldown(torch.from_numpy(video), order, return_info=True, combed=method, **k)
            assert got.device.type == "cuda" and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (fmt, order, method)
            _same_info(info, winfo)
            assert insert is None or info["combed"] == insert
        want, winfo = pd.remove_pulldown_frames(video, order, combed="yadif", comb_threshold=3, comb_pixels=8, **k)
        got, info = savsr_amd.remove_pulldown(torch.from_numpy(video).to(DEV), order, return_info=True, combed="yadif", comb_threshold=3, comb_pixels=8, **k)
        assert np.array_equal(got.cpu().numpy(), want)
        _same_info(info, winfo)


def test_combed_changes_nothing_on_clean_film_and_none_is_the_call_without_it():
    video = pd.telecine(packed_film("gradient", 8, H, W), "tff")
    plain, pinfo = savsr_amd.remove_pulldown(torch.from_numpy(video), "tff", return_info=True)
    assert sorted(pinfo) == ["kept", "matches", "sad", "scores"]
    got, info = savsr_amd.remove_pulldown(torch.from_numpy(video), "tff", return_info=True, combed="bwdif")
    assert torch.equal(got, plain) and info["combed"] == [] and not info["comb"].any()
    none, ninfo = savsr_amd.remove_pulldown(torch.from_numpy(video), "tff", return_info=True, combed=None)
    assert torch.equal(none, plain) and sorted(ninfo) == sorted(pinfo)


# ---------------------------------------------------------------------------------------------------------------------- the property
@pytest.mark.parametrize("method", DEINTERLACERS)
def test_property_on_the_hybrid(net3, method):
    """upscale_video(v, pulldown=o, combed=m) is upscale_video on remove_pulldown(v, o, combed=m), the spec's and the GPU's."""
    video, insert = cc.hybrid("tff", H, W)
    film = pd.remove_pulldown_frames(video, "tff", combed=method)[0]
    on_gpu = savsr_amd.remove_pulldown(torch.from_numpy(video), "tff", combed=method)
    assert np.array_equal(on_gpu.cpu().numpy(), film) and film.shape[0] == 21
    want = net3.upscale_video(torch.from_numpy(film), scale=2, out="uint8")
    got = net3.upscale_video(torch.from_numpy(video), scale=2, out="uint8", pulldown="tff", combed=method)
    assert got.shape == want.shape and torch.equal(got, want)
    plain = net3.upscale_video(torch.from_numpy(video), scale=2, out="uint8", pulldown="tff")
    # without combed= the insert goes into the network combed; the frames whose windows end before it are the same either way
    assert not torch.equal(got, plain) and torch.equal(got[:4], plain[:4]) and insert[0] == 10


def test_property_i420_with_parameters_and_scan_detect(net3):
    video, _ = cc.hybrid("bff", H, W, fmt="i420")
    kw = dict(pixel_format="i420", size=(H, W))
    film = savsr_amd.remove_pulldown(torch.from_numpy(video), "bff", combed="yadif", comb_threshold=6, comb_pixels=24, **kw)
    want = net3.upscale_video(film, scale=2, out="i420", **kw)
    got = net3.upscale_video(torch.from_numpy(video), scale=2, out="i420", pulldown="bff", combed="yadif", comb_threshold=6, comb_pixels=24, **kw)
    assert torch.equal(got, want)
    # scan="detect": combed= says how a telecine verdict is carried out and is ignored for the others
    clean = pd.telecine(cc.packed("sinusoid", 16, H, W), "tff")
    verdict = savsr_amd.detect_scan(torch.from_numpy(clean))
    found = verdict.kwargs()
    more = dict(combed="bwdif") if "pulldown" in found else {}
    assert torch.equal(net3.upscale_video(torch.from_numpy(clean), scale=2, out="uint8", scan="detect", combed="bwdif"),
                       net3.upscale_video(torch.from_numpy(clean), scale=2, out="uint8", **found, **more))
    flat = torch.full((8, H, W, 3), 90, dtype=torch.uint8)                            # undetermined: no stage, combed= ignored
    assert torch.equal(net3.upscale_video(flat, scale=2, out="uint8", scan="detect", combed="bwdif"), net3.upscale_video(flat, scale=2, out="uint8"))


# ---------------------------------------------------------------------------------------------------------------------- streaming
@pytest.mark.parametrize("chunk", [1, 3, 7, 26])
def test_video_upscaler_with_combed_any_chunking_is_bitwise(net3, chunk):
    from savsr_amd import VideoUpscaler
    video, insert = cc.hybrid("tff", H, W)
    n = video.shape[0]
    u8 = torch.from_numpy(video)
    whole, winfo = savsr_amd.remove_pulldown(u8, "tff", return_info=True, combed="bwdif")
    whole8 = net3.upscale_video(u8, scale=2, out="uint8", pulldown="tff", combed="bwdif")
    up = VideoUpscaler(net3, 2, out="uint8", pulldown="tff", combed="bwdif")
    parts = []
    for a in range(0, n, chunk):
        parts.append(up.push(u8[a:a + chunk]))
        rem = up._split
        assert 1 <= rem.held <= 5 + 3 and rem._wov.shape[0] <= 2 and (rem._pend is None or rem._pend.shape[0] <= 4)          # two more than without combed=
        for t in (rem._ctx, rem._last, rem._pend, rem._wov):                          # copies of their own: the chunk's storage is released
            assert t is None or t.untyped_storage().nbytes() == t.numel() * t.element_size()
    parts.append(up.finish())
    assert all(p.shape[1:] == whole8.shape[1:] for p in parts)
    assert torch.equal(torch.cat(parts, 0), whole8) and up._buf is None and up._split.held == 0
    assert up.pulldown_info == {"matches": winfo["matches"], "kept": winfo["kept"], "combed": insert} and whole.shape[0] == 21
    if chunk == 3:                                                                    # planar, another cycle, cuts and a crop behind the stage
        yv, _ = cc.hybrid("bff", H, W, fmt="i420", depth=10, parts=(4, 3, 4))
        yv = torch.from_numpy(yv)
        kw = dict(out="i420", pixel_format="i420", size=(H, W), depth=10, out_depth=10)
        more = dict(pulldown="bff", pulldown_cycle=4, combed="yadif", comb_pixels=30, cuts="auto", crop=(2, 4, 11, 12))
        whole = net3.upscale_video(yv, scale=2, **more, **kw)
        up = VideoUpscaler(net3, 2, **more, **kw)
        parts = [up.push(yv[a:a + chunk]) for a in range(0, yv.shape[0], chunk)] + [up.finish()]
        assert torch.equal(torch.cat(parts, 0), whole) and up.pulldown_info["combed"] == [5, 6, 7]


# ---------------------------------------------------------------------------------------------------------------------- the CLI
def test_cli_y4m_combed(net3, tmp_path, capsys):
    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    frames, insert = cc.hybrid("tff", H, W, fmt="i420")
    f = io.BytesIO()
    y4m.Y4MWriter(f, W, H, (30000, 1001), "t", (1, 1)).write(frames)
    src, ckpt, dst = tmp_path / "lr.y4m", tmp_path / "net.pth", tmp_path / "sr.y4m"
    src.write_bytes(f.getvalue())
    sio.save_network(net3, str(ckpt))
    kw = dict(out="i420", pixel_format="i420", size=(H, W))
    assert main(["-i", str(src), "--scale", "2", "--checkpoint", str(ckpt), "--chunk", "4", "-o", str(dst), "--pulldown", "auto", "--combed", "bwdif"]) == 0
    sr = net3.upscale_video(torch.from_numpy(frames), scale=2, pulldown="tff", combed="bwdif", **kw)
    g = io.BytesIO()
    y4m.Y4MWriter(g, 2 * W, 2 * H, (24000, 1001), "p", y4m.scaled_aspect((1, 1), (H, W), (2 * H, 2 * W))).write(sr.cpu().numpy())
    assert sr.shape[0] == 21 and dst.read_bytes() == g.getvalue()
    cap = capsys.readouterr()
    assert "--combed bwdif: 6 of 26 woven frames were combed and deinterlaced" in cap.err
    assert "pulldown tff: 26 frames in, 21 out" in cap.out
