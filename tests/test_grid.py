"""The grid origin of the deblocking rule and the grid detector, on the host (savsr_amd/deblock.py, savsr_amd/grid.py): the padding identity
that defines an origin, the statistics on hand-made lines, the decision on the 288 x 352 set of tests/grid_cases.py (every case
required), every refusal by name, the option plumbing of upscale_video / VideoUpscaler / the command line, the header / binding / library
at ABI 53, and the sanitizer host check of the kernels' code."""
import os
import re
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import savsr_amd
from savsr_amd import _lib
from savsr_amd import deblock as db
from savsr_amd import grid as G
from tests.deblock_cases import BLOCKS, COVER_SHAPE, MODES, case_frames, case_plane
from tests.grid_cases import BLOCKY, CLEAN_SIGMAS, DECISION_SHAPE, blocky, case_seed, origins, uniform_noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cover():
    return case_plane(np.random.default_rng(11), *COVER_SHAPE)


# ---------------------------------------------------------------------------------------------------------------------- the origin
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("block", BLOCKS)
def test_an_origin_is_the_rule_on_the_padded_plane(cover, block, mode):
    """deblock_matrix(m, origin) == deblock_matrix(pad(m, edge))[pad:]: every origin of every block, both modes; field-wise with even oy."""
    for oy in range(block):
        for ox in range(block):
            py, px = (block - oy) % block, (block - ox) % block
            want = db.deblock_matrix(np.pad(cover, ((py, 0), (px, 0)), mode="edge"), 8, block, block, mode)[py:, px:]
            assert np.array_equal(db.deblock_matrix(cover, 8, block, block, mode, origin_y=oy, origin_x=ox), want), (oy, ox)
            assert np.array_equal(db.deblock_plane(cover, 8, block, mode, origin=(oy, ox)), want)
            if oy % 2 == 0:
                got = db.deblock_fields(cover, 8, block, mode, origin=(oy, ox))
                fy = (block // 2 - oy // 2) % (block // 2)
                for p in (0, 1):
                    f = np.pad(cover[p::2], ((fy, 0), (px, 0)), mode="edge")
                    assert np.array_equal(got[p::2], db.deblock_matrix(f, 8, block // 2, block, mode)[fy:, px:]), (oy, ox, p)
                assert np.array_equal(db.deblock_plane(cover, 8, block, mode, interlaced=True, origin=(oy, ox)), got)
    m16 = case_plane(np.random.default_rng(12), 21, 35, 12, above=True)
    want = db.deblock_matrix(np.pad(m16, ((5, 0), (3, 0)), mode="edge"), 12, 8, 8, mode)[5:, 3:]
    assert np.array_equal(db.deblock_matrix(m16, 12, 8, 8, mode, origin_y=3, origin_x=5), want)


def test_origin_zero_is_the_rule_as_it_stands(cover):
    for block in BLOCKS:
        for mode in MODES:
            a = db.deblock_matrix(cover, 8, block, block, mode)
            assert np.array_equal(a, db.deblock_matrix(cover, 8, block, block, mode, origin_y=0, origin_x=0))
            assert np.array_equal(db.deblock_plane(cover, 8, block, mode, origin=(0, 0)), a)
            assert np.array_equal(db.deblock_fields(cover, 8, block, mode), db.deblock_fields(cover, 8, block, mode, origin=(0, 0)))
    out, counts = db.deblock_matrix(cover, 8, 8, 8, "strong", return_counts=True, origin_y=1, origin_x=1)
    assert counts["dropped"] > 0 and counts["filtered"] > 0          # P2 of the edge at 1 lies beyond the plane: its write is dropped


def test_the_p_side_beyond_the_plane():
    """Edges at e = 1 and 2: P1 / P2 read the first sample, their writes are dropped; a plane of one sample has no edge."""
    line = np.array([[100, 104, 104, 104, 104, 104, 104, 104, 104, 104]], np.uint8)
    got = db.deblock_matrix(line, 8, 8, 8, "strong", (255, 255), origin_x=1)          # delta = 4: t(2) = 2, t(4) = 1, t(8) = 0
    assert got[0].tolist() == [102, 102, 103, 104, 104, 104, 104, 104, 104, 104]
    assert np.array_equal(db.deblock_matrix(np.array([[7]], np.uint8), origin_y=1, origin_x=1), [[7]])


def test_deblock_frames_with_origins():
    rng = np.random.default_rng(13)
    v = case_frames(rng, 2, 19, 27, step=3)
    want = np.stack([np.stack([db.deblock_plane(v[t, :, :, c], origin=(3, 5)) for c in range(3)], -1) for t in range(2)])
    assert np.array_equal(db.deblock_frames(v, origin=(3, 5)), want) and not np.array_equal(want, db.deblock_frames(v))
    from savsr_amd import yuv
    h, w = 20, 38
    planes = [case_frames(rng, 2, *hw)[..., 0] for hw in [(h, w)] + [yuv.chroma_hw(h, w, "420")] * 2]
    frames = np.concatenate([p.reshape(2, -1) for p in planes], 1)
    got = db.deblock_frames(frames, "i420", (h, w), origin=(2, 5), chroma_origin=(1, 6))
    parts = [np.stack([db.deblock_plane(p[t], origin=o) for t in range(2)]).reshape(2, -1) for p, o in zip(planes, ((2, 5), (1, 6), (1, 6)))]
    assert np.array_equal(got, np.concatenate(parts, 1))
    f444 = np.concatenate([case_frames(rng, 1, 12, 18)[..., 0].reshape(1, -1) for _ in range(3)], 1)
    assert np.array_equal(db.deblock_frames(f444, "i444", (12, 18), origin=(3, 3)), db.deblock_frames(f444, "i444", (12, 18), origin=(3, 3), chroma_origin=(3, 3)))
    # chunking: the rule is stateless, so any split of the video gives the same bytes
    whole = db.deblock_frames(v, origin=(3, 5), interlaced=False)
    assert np.array_equal(np.concatenate([db.deblock_frames(v[:1], origin=(3, 5)), db.deblock_frames(v[1:], origin=(3, 5))]), whole)


# ---------------------------------------------------------------------------------------------------------------------- the statistics
def _row(values, **kw):
    return G.grid_stats_matrix(np.array([values], np.uint8 if max(values) < 256 else np.uint16), **kw)[0]


def test_stats_on_hand_made_lines():
    assert _row([10, 10, 14, 14]).tolist() == [0, 0, 1] + [0] * 13          # a single step at x = 2
    assert _row([10, 10, 10, 14, 14]).tolist() == [0, 0, 0, 1] + [0] * 12
    assert not _row([10, 12, 16, 18]).any()          # s = 4 = l + r exactly: not a hit
    assert _row([10, 12, 17, 19]).tolist()[2] == 1          # s = 5 > 4
    assert _row([0, 0, 32, 32]).tolist()[2] == 1 and not _row([0, 0, 33, 33]).any()          # s = cap and cap + 1
    assert _row([0, 0, 33, 33], cap=33).tolist()[2] == 1 and not _row([0, 0, 1, 1], cap=0).any()
    assert not _row([1, 9, 1]).any() and not _row([5]).any()          # lines of length 3 and 1: no boundary
    assert _row([9, 9, 1, 1]).tolist()[2] == 1          # length 4: the one boundary
    line = [50] * 40
    line[18:] = [54] * 22
    line[34:] = [50] * 6
    assert _row(line).tolist() == [0, 0, 2] + [0] * 13          # x = 18 and x = 34 land in cell 2
    # columns, and both at once
    m = np.array([[10, 10, 14, 14]] * 4, np.uint8)
    assert G.grid_stats_matrix(m).tolist() == [[0, 0, 4] + [0] * 13, [0] * 16]
    assert G.grid_stats_matrix(m.T).tolist() == [[0] * 16, [0, 0, 4] + [0] * 13]
    assert not G.grid_stats_matrix(np.zeros((3, 3), np.uint8)).any() and not G.grid_stats_matrix(np.zeros((1, 1), np.uint8)).any()


def test_stats_read_16_bit_samples_on_the_8_bit_scale():
    """min(s, 2^d - 1) >> (d - 8): 60000 reads as 255 at either depth, and steps below one 8-bit code vanish."""
    m = np.array([[400, 400, 416, 416], [400, 400, 403, 403], [1023, 1023, 60000, 60000], [960, 960, 60000, 60000]], np.uint16)
    got = G.grid_stats_matrix(m, 10)
    assert got[0].tolist() == [0, 0, 2] + [0] * 13          # rows 0 (100 -> 104) and 3 (240 -> 255); row 1 is flat at 8 bits, row 2 is 255 throughout
    assert np.array_equal(got, G.grid_stats_matrix(np.minimum(m, 1023) >> 2, 8))
    assert np.array_equal(G.grid_stats_matrix(m, 12), G.grid_stats_matrix(np.minimum(m, 4095) >> 4, 8))


def test_stats_field_wise_with_an_odd_row_count():
    rng = np.random.default_rng(14)
    m = rng.integers(90, 110, (9, 21)).astype(np.uint8)
    got = G.grid_stats_matrix(m, 8, True)
    assert np.array_equal(got[0], G.grid_stats_matrix(m)[0])          # the rows are unchanged
    assert np.array_equal(got[1], G.grid_stats_matrix(m[0::2])[1] + G.grid_stats_matrix(m[1::2])[1])          # 5 and 4 field rows
    assert got[1][4:].sum() == 0 and got[1][2:4].sum() > 0          # the top field has boundaries 2 and 3, the bottom field boundary 2
    assert G.grid_pairs(9, 21, True).tolist() == [[9, 9, 18, 18] + [9] * 12, [0, 0, 42, 21] + [0] * 12]          # x = 2 .. 19; field rows 2, 3 and 2
    assert G.grid_pairs(9, 21).tolist()[1] == [0, 0] + [21] * 6 + [0] * 8
    assert G.grid_pairs(40, 3).tolist()[0] == [0] * 16


def test_stats_of_frames_by_class():
    rng = np.random.default_rng(15)
    v = rng.integers(90, 110, (2, 12, 20, 3)).astype(np.uint8)
    got = G.grid_stats_frames(v)
    assert got.shape == (2, 2, 2, 16) and not got[:, 1].any()
    assert np.array_equal(got[1, 0], sum(G.grid_stats_matrix(v[1, :, :, c]) for c in range(3)))
    assert np.array_equal(G.frame_pairs(v.shape)[0], 3 * G.grid_pairs(12, 20)) and not G.frame_pairs(v.shape)[1].any()
    h, w = 12, 20
    y, cb, cr = (rng.integers(90, 110, (2,) + s).astype(np.uint8) for s in ((h, w), (6, 10), (6, 10)))
    frames = np.concatenate([p.reshape(2, -1) for p in (y, cb, cr)], 1)
    got = G.grid_stats_frames(frames, "i420", (h, w), interlaced=True)
    assert np.array_equal(got[0, 0], G.grid_stats_matrix(y[0], 8, True))
    assert np.array_equal(got[0, 1], G.grid_stats_matrix(cb[0], 8, True) + G.grid_stats_matrix(cr[0], 8, True))
    assert np.array_equal(G.frame_pairs(frames.shape, "i420", (h, w), 8, True)[1], 2 * G.grid_pairs(6, 10, True))
    assert not G.grid_stats_frames(frames[:, :h * w], "y400", (h, w))[:, 1].any()


# ---------------------------------------------------------------------------------------------------------------------- the decision
def _verdict(m, interlaced=False):
    table, pairs = np.zeros((2, 2, 16), np.int64), np.zeros((2, 2, 16), np.int64)
    table[0], pairs[0] = G.grid_stats_matrix(m, 8, interlaced), G.grid_pairs(*m.shape, interlaced)
    return G.verdict_from_stats(table, pairs, interlaced)


@pytest.mark.parametrize("block,a,sigma", BLOCKY)
def test_the_decision_finds_every_blocky_picture(block, a, sigma):
    for origin in origins(block):
        v = _verdict(blocky(case_seed(block, a, sigma, *origin), *DECISION_SHAPE, block, a, sigma, origin))
        assert (v.block, v.origin) == (block, origin), (origin, v.peaks)
        assert v.chroma_origin is None and v.kwargs() == dict(deblock_block=block, deblock_origin=origin)
        want = tuple(range(origin[1] % block, 16, block)), tuple(range(origin[0] % block, 16, block))
        assert v.peaks[0] == want and v.peaks[1] == ((), ())


def test_the_decision_finds_no_grid_in_unblocked_pictures():
    for sigma in CLEAN_SIGMAS:
        v = _verdict(blocky(case_seed(0, sigma), *DECISION_SHAPE, None, 0, sigma))
        assert v.block is None and v.origin is None and v.kwargs() == {}, (sigma, v.peaks)
    assert _verdict(uniform_noise(case_seed(99), *DECISION_SHAPE)).block is None


def test_the_decision_reads_a_frame_coded_picture_field_wise():
    """Block 8 in the frame is (8, ox) along the rows and block 4 at oy / 2 down either field."""
    for origin in ((0, 0), (2, 5), (6, 1)):
        m = blocky(case_seed(8, 4, 1, *origin, 1), *DECISION_SHAPE, 8, 4, 1, origin)
        v = _verdict(m, True)
        assert (v.block, v.origin) == (8, origin), (origin, v.peaks)
        assert v.peaks[0][1] == tuple(range(origin[0] // 2, 16, 4))
    m = blocky(case_seed(16, 4, 1, 4, 3, 1), *DECISION_SHAPE, 16, 4, 1, (4, 3))
    assert (_verdict(m, True).block, _verdict(m, True).origin) == (16, (4, 3))
    m = blocky(case_seed(4, 6, 2, 0, 1, 1), *DECISION_SHAPE, 4, 6, 2, (2, 1))          # block 4: the columns are not consulted
    assert (_verdict(m, True).block, _verdict(m, True).origin) == (4, (0, 1))


def test_the_rule_on_hand_made_tables():
    pairs = np.zeros((2, 2, 16), np.int64)
    pairs[0] = 1000
    flat = np.full(16, 100, np.int64)

    def table(rows, cols):
        t = np.zeros((2, 2, 16), np.int64)
        t[0, 0], t[0, 1] = rows, cols
        return t

    def peaks(*cells, base=flat, height=150):
        out = base.copy()
        out[list(cells)] = height
        return out

    v = G.verdict_from_stats(table(peaks(3, 11), peaks(7, 15)), pairs)          # exactly ratio x the median: a peak
    assert (v.block, v.origin) == (8, (7, 3)) and v.peaks[0] == ((3, 11), (7, 15))
    assert G.verdict_from_stats(table(peaks(3, 11, height=149), peaks(7, 15)), pairs).block is None
    assert G.verdict_from_stats(table(peaks(3, 11), peaks(7)), pairs).block is None          # 8 one way, 16 the other
    assert G.verdict_from_stats(table(peaks(3, 11), peaks(7, 14)), pairs).block is None          # not 8 apart
    assert G.verdict_from_stats(table(peaks(3, 11, 12), peaks(7, 15)), pairs).block is None          # a stray peak
    assert G.verdict_from_stats(table(peaks(5), peaks(0)), pairs).origin == (0, 5)
    assert G.verdict_from_stats(table(peaks(1, 5, 9, 13), peaks(2, 6, 10, 14)), pairs).origin == (2, 1)
    assert G.verdict_from_stats(table(peaks(3, 11), peaks(7, 15)), pairs, min_count=151).block is None
    assert G.verdict_from_stats(table(peaks(3, 11), peaks(7, 15)), pairs, ratio=Fraction(151, 100)).block is None
    hole = pairs.copy()
    hole[0, 1, 0] = 0
    assert G.verdict_from_stats(table(peaks(3, 11), peaks(7, 15)), hole).block is None          # an empty cell: no answer
    # interlaced: rows 8 with columns 4 at q gives oy = 2 q; rows 16 with columns 8; rows 4 alone
    assert G.verdict_from_stats(table(peaks(3, 11), peaks(1, 5, 9, 13)), pairs, True).origin == (2, 3)
    assert G.verdict_from_stats(table(peaks(3, 11), peaks(7, 15)), pairs, True).block is None
    assert G.verdict_from_stats(table(peaks(3), peaks(2, 10)), pairs, True).origin == (4, 3)
    v = G.verdict_from_stats(table(peaks(1, 5, 9, 13), flat), hole, True)
    assert (v.block, v.origin) == (4, (0, 1))
    # the chroma class: its origin where its block is the luma's, None elsewhere; kwargs say what to do with the chroma planes
    both = table(peaks(3, 11), peaks(7, 15))
    pairs2 = np.full((2, 2, 16), 1000, np.int64)
    both[1, 0], both[1, 1] = peaks(1, 9), peaks(4, 12)
    v = G.verdict_from_stats(both, pairs2)
    assert v.chroma_origin == (4, 1) and v.kwargs() == dict(deblock_block=8, deblock_origin=(7, 3), deblock_chroma_origin=(4, 1))
    both[1, 0] = peaks(1)
    v = G.verdict_from_stats(both, pairs2)
    assert v.block == 8 and v.chroma_origin is None
    assert v.kwargs() == dict(deblock_block=8, deblock_origin=(7, 3), deblock_chroma_origin=(0, 0), deblock_chroma_strength=(0, 0))
    assert v.as_json()["peaks"][0] == [[3, 11], [7, 15]] and v.as_json()["block"] == 8 and len(v.as_json()["table"][1][1]) == 16
    both[0, 0] = flat
    assert G.verdict_from_stats(both, pairs2).kwargs() == {}          # no luma grid: no grid


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_every_refusal_by_name(cover):
    for call, words in (
            (lambda: db.deblock_matrix(cover, origin_x=8), r"origin_x = 8: an int in 0 \.\. 7"),
            (lambda: db.deblock_matrix(cover, 8, 4, 8, origin_y=4), r"origin_y = 4: an int in 0 \.\. 3"),
            (lambda: db.deblock_matrix(cover, origin_y=-1), r"origin_y = -1"),
            (lambda: db.deblock_matrix(cover, origin_x=1.0), r"origin_x = 1\.0"),
            (lambda: db.deblock_fields(cover, origin=(3, 0)), r"origin = \(3, 0\): oy must be even on a field-wise run"),
            (lambda: db.deblock_plane(cover, interlaced=True, origin=(1, 1)), r"oy must be even"),
            (lambda: db.deblock_plane(cover, origin=(8, 0)), r"origin = \(8, 0\): two ints \(oy, ox\) in 0 \.\. 7"),
            (lambda: db.deblock_plane(cover, origin=3), r"origin = 3: two ints"),
            (lambda: db.deblock_plane(cover, 8, 4, origin=(0, 4)), r"origin = \(0, 4\): two ints \(oy, ox\) in 0 \.\. 3"),
            (lambda: db.deblock_frames(np.zeros((1, 24), np.uint8), "i420", (4, 4), origin=(1, 0)),
             r"origin = \(1, 0\) on 4:2:0 frames needs chroma_origin="),
            (lambda: db.deblock_frames(np.zeros((1, 32), np.uint8), "i422", (4, 4), origin=(0, 1)), r"on 4:2:2 frames needs chroma_origin="),
            (lambda: db.deblock_frames(np.zeros((1, 24), np.uint8), "i420", (4, 4), chroma_origin=(0, 9)), r"chroma_origin = \(0, 9\)"),
            (lambda: db.deblock_frames(np.zeros((1, 24), np.uint8), "i420", (4, 4), interlaced=True, origin=(2, 0), chroma_origin=(1, 0)),
             r"chroma_origin = \(1, 0\): oy must be even"),
            (lambda: G.grid_stats_matrix(cover, cap=256), r"cap = 256: an int in 0 \.\. 255"),
            (lambda: G.grid_stats_matrix(cover, cap=-1), r"cap = -1"),
            (lambda: G.grid_stats_matrix(cover.astype(np.float32)), r"the matrix must be \[R, C\] integers"),
            (lambda: G.grid_stats_matrix(cover, 9), r"depth = 9: 8, 10 or 12"),
            (lambda: G.grid_stats_matrix(np.zeros((0, 4), np.uint8)), r"a matrix of 0 x 4"),
            (lambda: G.grid_stats_frames(np.zeros((1, 3, 4, 4), np.float32)), r"float frames have no integer samples to find a grid in"),
            (lambda: G.grid_stats_frames(np.zeros((1, 23), np.uint8), "i420", (4, 4)), r"are \[N, 24\] uint8"),
            (lambda: G.verdict_from_stats(np.zeros((2, 16), np.int64), np.zeros((2, 2, 16), np.int64)), r"table and pairs are \[2, 2, 16\] integers"),
            (lambda: G.verdict_from_stats(np.zeros((2, 2, 16), np.int64), np.zeros((2, 2, 16), np.int64), ratio=1), r"ratio = 1: a finite number above 1"),
            (lambda: G.verdict_from_stats(np.zeros((2, 2, 16), np.int64), np.zeros((2, 2, 16), np.int64), ratio="x"), r"ratio = 'x'"),
            (lambda: G.verdict_from_stats(np.zeros((2, 2, 16), np.int64), np.zeros((2, 2, 16), np.int64), min_count=0), r"min_count = 0: an int >= 1")):
        with pytest.raises(ValueError, match=words):
            call()
    # i444, y400 and packed frames: None means the same origin
    db.deblock_frames(np.zeros((1, 48), np.uint8), "i444", (4, 4), origin=(1, 1))
    db.deblock_frames(np.zeros((1, 16), np.uint8), "y400", (4, 4), origin=(1, 1))
    db.deblock_frames(np.zeros((1, 4, 4, 3), np.uint8), origin=(1, 1))


def test_the_video_calls_refuse_before_the_gpu_is_touched():
    """upscale_video / VideoUpscaler on a network that is not on a GPU: every refusal is raised on the host, before the call would have
    asked for the device (a good call ends at that question)."""
    from savsr_amd import VideoUpscaler
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR(num_feat=32).eval()
    v = torch.zeros(8, 12, 16, 3, dtype=torch.uint8)
    calls = (lambda **kw: net.upscale_video(v, scale=2, out="uint8", **kw), lambda **kw: VideoUpscaler(net, 2, out="uint8", **kw))
    for call in calls:
        for kw, words in ((dict(deblock_origin=(1, 1)), r"deblock_origin = \(1, 1\) goes with deblock="),
                          (dict(deblock_chroma_origin=(0, 0)), r"deblock_chroma_origin = \(0, 0\) goes with deblock="),
                          (dict(deblock="weak", deblock_grid="yes"), r"deblock_grid = 'yes': None or 'auto'"),
                          (dict(deblock="weak", deblock_origin=(8, 0)), r"deblock_origin = \(8, 0\): two ints \(oy, ox\) in 0 \.\. 7"),
                          (dict(deblock="weak", deblock_block=4, deblock_origin=(0, 4)), r"deblock_origin = \(0, 4\)"),
                          (dict(deblock="weak", deblock_origin=(1.0, 0)), r"deblock_origin = \(1\.0, 0\)"),
                          (dict(deblock="weak", deblock_chroma_origin=(0, -1)), r"deblock_chroma_origin = \(0, -1\)"),
                          (dict(deblock="weak", fields="tff", deblock_origin=(3, 0)), r"deblock_origin = \(3, 0\): oy must be even"),
                          (dict(deblock="weak", pulldown="tff", deblock_origin=(2, 0), deblock_chroma_origin=(5, 0)),
                           r"deblock_chroma_origin = \(5, 0\): oy must be even")):
            with pytest.raises(ValueError, match=words):
                call(**kw)
    for kw, words in ((dict(deblock_grid="auto"), r"deblock_grid = 'auto' goes with deblock="),
                      (dict(deblock="weak", deblock_grid="auto", deblock_block=16), r"deblock_block = 16 together with deblock_grid = 'auto'"),
                      (dict(deblock="weak", deblock_grid="auto", deblock_origin=(1, 0)), r"deblock_origin = \(1, 0\) together with deblock_grid = 'auto'"),
                      (dict(deblock="weak", deblock_grid="auto", deblock_chroma_origin=(0, 0)), r"deblock_chroma_origin = \(0, 0\) together with")):
        with pytest.raises(ValueError, match=words):
            net.upscale_video(v, scale=2, out="uint8", **kw)
    with pytest.raises(ValueError, match=r"deblock_grid = 'auto' in VideoUpscaler: the decision needs the whole video"):
        VideoUpscaler(net, 2, out="uint8", deblock="weak", deblock_grid="auto")
    y = torch.zeros(8, 12 * 16 * 3 // 2, dtype=torch.uint8)
    fmt = dict(pixel_format="i420", size=(12, 16), out="i420")
    with pytest.raises(ValueError, match=r"deblock_origin = \(1, 0\) on 4:2:0 frames needs deblock_chroma_origin="):
        net.upscale_video(y, scale=2, deblock="weak", deblock_origin=(1, 0), **fmt)
    with pytest.raises(ValueError, match="float frames"):
        net.upscale_video(torch.zeros(8, 3, 12, 16), scale=2, deblock="weak", deblock_grid="auto")
    with pytest.raises(TypeError):                                                   # keyword only
        net.upscale_video(v, 2, "reflection", "uint8", "rgb", None, None, 10.0, "bt601", None, 8, None, None, None, None, None, 24, "keep", None, None, 5,
                          (1, 1))
    for kw in (dict(deblock="strong", deblock_origin=(7, 7)), dict(deblock="strong", deblock_grid="auto"),
               dict(deblock="weak", fields="bff", deblock_origin=(6, 7), deblock_chroma_origin=(0, 1))):
        with pytest.raises(RuntimeError, match="AMD GPU only"):                      # a good call gets as far as the device
            net.upscale_video(v, scale=2, out="uint8", **kw)
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        net.upscale_video(y, scale=2, deblock="weak", deblock_origin=(1, 0), deblock_chroma_origin=(3, 3), **fmt)
    for call, words in ((lambda: savsr_amd.deblock_video(v, origin=(0, 8)), r"origin = \(0, 8\)"),
                        (lambda: savsr_amd.deblock_video(v, interlaced=True, origin=(1, 0)), r"oy must be even"),
                        (lambda: savsr_amd.deblock_video(y, "i420", (12, 16), origin=(1, 1)), r"needs chroma_origin="),
                        (lambda: savsr_amd.grid_stats(torch.zeros(2, 3, 4, 4)), r"float frames have no integer samples to find a grid in"),
                        (lambda: savsr_amd.grid_stats(v, cap=300), r"cap = 300"),
                        (lambda: savsr_amd.detect_grid(v, ratio=0.5), r"ratio = 0\.5"),
                        (lambda: savsr_amd.detect_grid(v, min_count=0), r"min_count = 0"),
                        (lambda: savsr_amd.detect_grid(torch.zeros(2, 3, 4, 4)), r"float frames")):
        with pytest.raises(ValueError, match=words):
            call()


def test_the_stage_in_video_upscaler_stays_stateless():
    """The origins are two more checked options that push() hands the stage with the chunk it was given: nothing is held back, so any
    chunking gives the same bytes (the numpy side of that: `deblock_frames` of the chunks is `deblock_frames` of the video)."""
    from savsr_amd import VideoUpscaler
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR(num_feat=32).eval()
    up = VideoUpscaler(net, 2, out="uint8", deblock="strong", deblock_origin=(3, 5))
    assert up._edges == (8, "strong", (25, 13), (25, 13)) and up._grid == ((3, 5), (3, 5)) and up._noise is None and up._split is None and up._buf is None
    assert VideoUpscaler(net, 2, out="uint8", deblock="weak")._grid == ((0, 0), (0, 0)) and VideoUpscaler(net, 2, out="uint8")._grid is None
    up = VideoUpscaler(net, 2, pixel_format="i420", size=(12, 16), out="i420", deblock="weak", fields="tff", deblock_origin=(2, 1), deblock_chroma_origin=(4, 0))
    assert up._grid == ((2, 1), (4, 0)) and up._fieldwise
    v = case_frames(np.random.default_rng(16), 5, 19, 27, step=3)
    whole = db.deblock_frames(v, mode="strong", origin=(3, 5))
    for chunk in (1, 2, 5):
        assert np.array_equal(np.concatenate([db.deblock_frames(v[a:a + chunk], mode="strong", origin=(3, 5)) for a in range(0, 5, chunk)]), whole)


# ---------------------------------------------------------------------------------------------------------------------- the CLI
def test_cli_arguments(capsys):
    from savsr_amd.upscale import deblock_kwargs, parse_args
    base = ["-i", "in.y4m", "-o", "out.y4m", "--scale", "2", "--checkpoint", "x.pth"]
    a = parse_args(base + ["--deblock", "weak"])
    assert a.deblock_origin == (0, 0) and a.deblock_chroma_origin is None and a.deblock_grid is None and "deblock_origin" not in deblock_kwargs(a)
    a = parse_args(base + ["--deblock", "strong", "--deblock-origin", "3,5", "--deblock-chroma-origin", "6, 2"])
    assert deblock_kwargs(a) == dict(deblock="strong", deblock_block=8, deblock_strength=(25, 13), deblock_chroma_strength=None, deblock_origin=(3, 5),
                                     deblock_chroma_origin=(6, 2))
    a = parse_args(base + ["--deblock", "strong", "--deblock-grid", "auto", "--grid-out", "g.json", "--scan", "detect", "--crop", "auto"])
    assert a.deblock_grid == "auto" and a.grid_out == "g.json" and a.deblock_block == 8
    png = ["-i", "in", "-o", "out", "--scale", "2", "--checkpoint", "x.pth"]
    assert parse_args(png + ["--deblock", "weak", "--deblock-block", "16", "--deblock-origin", "15,9"]).deblock_origin == (15, 9)
    assert parse_args(png + ["--deblock", "weak", "--deblock-grid", "auto"]).deblock_grid == "auto"
    for extra, words in ((["--deblock-origin", "1,1"], "go with --deblock weak or strong"),
                         (["--deblock", "none", "--deblock-grid", "auto"], "go with --deblock weak or strong"),
                         (["--grid-out", "g.json"], "--grid-out goes with --deblock-grid auto"),
                         (["--deblock", "weak", "--grid-out", "g.json"], "--grid-out goes with --deblock-grid auto"),
                         (["--deblock", "weak", "--deblock-grid", "auto", "--deblock-block", "8"], "give one or the other"),
                         (["--deblock", "weak", "--deblock-grid", "auto", "--deblock-origin", "0,0"], "give one or the other"),
                         (["--deblock", "weak", "--deblock-grid", "manual"], "invalid choice"),
                         (["--deblock", "weak", "--deblock-origin", "8,0"], "--deblock-origin = (8, 0): two ints (oy, ox) in 0 .. 7"),
                         (["--deblock", "weak", "--deblock-block", "4", "--deblock-origin", "0,4"], "--deblock-origin = (0, 4)"),
                         (["--deblock", "weak", "--deblock-origin", "3"], "--deblock-origin = '3': Y,X"),
                         (["--deblock", "weak", "--deblock-origin", "a,b"], "--deblock-origin = 'a,b': Y,X"),
                         (["--deblock", "weak", "--deblock-chroma-origin", "0,-1"], "--deblock-chroma-origin = (0, -1)")):
        with pytest.raises(SystemExit):
            parse_args(base + extra)
        assert words in capsys.readouterr().err, extra
    with pytest.raises(SystemExit):
        parse_args(png + ["--deblock", "weak", "--deblock-chroma-origin", "2,2"])
    assert "--deblock-chroma-origin goes with a Y4M input" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(["-i", "-", "-o", "out.y4m", "--scale", "2", "--checkpoint", "x.pth", "--deblock", "weak", "--deblock-grid", "auto"])
    assert "--deblock-grid auto needs a first pass over the input, which stdin does not allow" in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------------------------------- the ABI
def test_header_binding_and_library_agree_at_abi_53():
    hdr = open(os.path.join(ROOT, "include", "savsr_hip.h")).read()
    assert int(re.search(r"#define\s+SAVSR_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 53
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    assert lib.savsr_abi_version() == _lib.ABI_VERSION
    for name in ("savsr_video_deblock_u8_o", "savsr_video_deblock_u16_o", "savsr_video_grid_stats_u8", "savsr_video_grid_stats_u16"):
        decl = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, plain, flags=re.S)
        assert decl, name
        params = [p.strip() for p in decl.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert len(params) == len(args), (name, params)
        for p, t in zip(params, args):          # pointers travel as void pointers, int64_t as c_int64, int as c_int
            want = _lib.C.c_void_p if "*" in p else _lib.C.c_int64 if p.startswith("int64_t") else _lib.C.c_int
            assert t is want, (name, p)
        assert hasattr(lib, name)
    names = [p.split()[-1].lstrip("*") for p in re.search(r"savsr_video_grid_stats_u16\s*\((.*?)\);", plain, flags=re.S).group(1).split(",")]
    assert names == ["frames", "n_frames", "frame_bytes", "plane_offset", "rows", "cols", "step", "depth", "interlaced", "cap", "out", "stream"]
    names = [p.split()[-1].lstrip("*") for p in re.search(r"savsr_video_deblock_u8_o\s*\((.*?)\);", plain, flags=re.S).group(1).split(",")]
    assert names[-3:] == ["origin_y", "origin_x", "stream"]
    build = open(os.path.join(ROOT, "savsr_amd", "csrc", "build.sh")).read()
    assert build.count("grid.hip") == 2
    assert callable(savsr_amd.grid_stats) and callable(savsr_amd.detect_grid) and savsr_amd.grid is G and savsr_amd.GridVerdict is G.GridVerdict
    # the entries refuse on the host, by name, before the device is touched
    assert lib.savsr_video_grid_stats_u8(0, 1, 1, 0, 1, 1, 1, 0, 32, 0, None) == -1
    assert b"video_grid_stats_u8: null pointer" in lib.savsr_last_error()
    buf = (_lib.C.c_uint8 * 512)()
    p = _lib.C.addressof(buf)
    q = (p + 256 + 7) // 8 * 8
    for args, words in (((p, 1, 64, 0, 8, 8, 1, 0, 256, q), b"video_grid_stats_u8: cap 0 .. 255"),
                        ((p, 1, 64, 0, 8, 8, 1, 0, 32, q + 4), b"video_grid_stats_u8: out must be 8-byte aligned"),
                        ((p, 1, 64, 0, 8, 8, 5, 0, 32, q), b"video_grid_stats_u8: step 1 .. 4")):
        assert lib.savsr_video_grid_stats_u8(*args, None) == -1 and words in lib.savsr_last_error(), args
    assert lib.savsr_video_deblock_u8_o(p, 1, 64, 0, 8, 8, 1, 8, 0, 0, 25, 13, p + 128, 64, 0, 8, 0, None) == -1
    assert b"video_deblock_u8_o: origin_y and origin_x 0 .. block - 1" in lib.savsr_last_error()
    assert lib.savsr_video_deblock_u8_o(p, 1, 64, 0, 8, 8, 1, 8, 0, 1, 25, 13, p + 128, 64, 0, 1, 0, None) == -1
    assert b"video_deblock_u8_o: origin_y even with interlaced" in lib.savsr_last_error()


# ---------------------------------------------------------------------------------------------------------------------- the host check
CXX = os.environ.get("CXX") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++"))


@pytest.mark.skipif(not CXX, reason="no clang++: the sanitizer build of the kernels' code needs one")
def test_the_kernels_code_passes_the_sanitizer_host_check():
    """tools/check_grid_host.py: csrc/grid.hip's entries and device functions and the origin path of csrc/deblock.hip as a stand-alone host
    program under ASan / UBSan, against the specifications (the tool's docstring says what the host form covers and what only the GPU
    tests do)."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_grid_host.py"), "--cxx", CXX], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "cases equal the specification or are refused by name, no sanitizer report" in res.stdout
