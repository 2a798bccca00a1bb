"""CPU checks of the deblocking stage: the rule of savsr_amd/deblock.py against a line-by-line restatement and what follows from it
(constant planes, a = 0, the bound on a sample's movement per pass and for both, the conserved sum, the flips, transposition and the
order of the passes), the hand-worked line, field-wise filtering, the coverage of the shared case generator, blocking reduced on a
synthetic picture, option checks and refusal messages, the command line's parsing, the stage's place in VideoUpscaler (stateless), the
header / binding / library at ABI 52, and the sanitizer host check of the kernels' code."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import savsr_amd
from savsr_amd import _lib
from savsr_amd import deblock as db
from tests.deblock_cases import BLOCKS, COVER_SHAPE, DEPTHS, MODES, as_bytes, blocky_picture, case_frames, case_plane, noise_plane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _naive_pass(v, block, strong, A, Bt, top, backwards=False):
    """One pass along the rows of v, edge by edge and line by line in place, straight from the module's docstring."""
    R, C = v.shape
    v = v.copy()
    t = lambda d, n: (abs(d) >> n) * (1 if d > 0 else -1)          # noqa: E731
    edges = list(range(block, C, block))
    for e in (reversed(edges) if backwards else edges):
        for y in range(R):
            s = [int(v[y, min(e + o, C - 1)]) for o in (-3, -2, -1, 0, 1, 2)]
            d = s[3] - s[2]
            if not (abs(d) < A and abs(s[2] - s[1]) < Bt and abs(s[3] - s[4]) < Bt):
                continue
            if strong:
                if not (abs(s[1] - s[0]) < Bt and abs(s[4] - s[5]) < Bt):
                    continue
                new = {-3: s[0] + t(d, 3), -2: s[1] + t(d, 2), -1: s[2] + t(d, 1), 0: s[3] - t(d, 1), 1: s[4] - t(d, 2), 2: s[5] - t(d, 3)}
            else:
                new = {-2: s[1] + t(d, 3), -1: s[2] + t(d, 1), 0: s[3] - t(d, 1), 1: s[4] - t(d, 3)}
            for o, val in new.items():
                if e + o <= C - 1:
                    v[y, e + o] = min(max(val, 0), top)
    return v


def _naive(m, depth, block_y, block_x, mode, thr, backwards=False):
    top, sh = (1 << depth) - 1, depth - 8
    v = np.minimum(m.astype(np.int64), top)
    v = _naive_pass(v, block_x, mode == "strong" and block_x >= 8, thr[0] << sh, thr[1] << sh, top, backwards)
    if block_y >= 4:
        v = _naive_pass(v.T, block_y, mode == "strong" and block_y >= 8, thr[0] << sh, thr[1] << sh, top, backwards).T
    return v.astype(m.dtype)


# ---------------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", DEPTHS)
def test_the_vectorised_rule_is_the_line_by_line_one_in_either_edge_order(depth, mode):
    """Edges of one pass never touch each other's samples, so taking them first to last or last to first in place gives the bytes of
    the vectorised form, which reads every edge from the pass's input."""
    rng = np.random.default_rng(depth)
    for (r, c), by, bx in (((19, 27), 8, 8), ((9, 9), 8, 8), ((21, 22), 4, 4), ((20, 35), 4, 8), ((33, 34), 16, 16), ((12, 17), 2, 4), ((1, 9), 8, 8)):
        for m in (case_plane(rng, r, c, depth, above=True, block=bx), noise_plane(rng, r, c, depth)):
            for thr in ((25, 13), (255, 255)):
                got = db.deblock_matrix(m, depth, by, bx, mode, thr)
                assert got.dtype == m.dtype and got.shape == m.shape
                assert np.array_equal(got, _naive(m, depth, by, bx, mode, thr)), (r, c, by, bx, thr)
                assert np.array_equal(got, _naive(m, depth, by, bx, mode, thr, backwards=True)), (r, c, by, bx, thr)


def test_the_hand_worked_line():
    """.. 255 255 247 | 255 255 255 .. under strong with thresholds 255: delta = 8, t(8) = 1, t(4) = 2, t(2) = 4; P2 and P1 leave the range
    and are clamped.  Weak moves P1, P0, Q0, Q1 alone."""
    line = np.full((1, 16), 255, np.uint8)
    line[0, 7] = 247
    got = db.deblock_matrix(line, 8, 8, 8, "strong", (255, 255))
    assert got[0, 5:11].tolist() == [255, 255, 251, 251, 253, 254] and (got[0, :5] == 255).all() and (got[0, 11:] == 255).all()
    got = db.deblock_matrix(line, 8, 8, 8, "weak", (255, 255))
    assert got[0, 5:11].tolist() == [255, 255, 251, 251, 254, 255]
    down = db.deblock_matrix(np.ascontiguousarray(line.T), 8, 8, 8, "strong", (255, 255))
    assert down[5:11, 0].tolist() == [255, 255, 251, 251, 253, 254]
    low = np.zeros((1, 16), np.uint8)
    low[0, 7] = 8          # delta = -8: truncation toward zero gives -1, -2, -4
    assert db.deblock_matrix(low, 8, 8, 8, "strong", (255, 255))[0, 5:11].tolist() == [0, 0, 4, 4, 2, 1]
    odd = np.zeros((1, 16), np.uint8)
    odd[0, 8:] = 7         # delta = 7: 7 >> 1 = 3, 7 >> 2 = 1, 7 >> 3 = 0; mirrored, the same magnitudes (toward zero, not floor)
    assert db.deblock_matrix(odd, 8, 8, 8, "strong", (255, 255))[0, 5:11].tolist() == [0, 1, 3, 4, 6, 7]
    assert db.deblock_matrix(odd[:, ::-1].copy(), 8, 8, 8, "strong", (255, 255))[0, 5:11].tolist() == [7, 6, 4, 3, 1, 0]


@pytest.mark.parametrize("mode", MODES)
def test_constant_planes_and_a_zero(mode):
    for depth in DEPTHS:
        top = (1 << depth) - 1
        for val in (0, 77 << (depth - 8), top):
            m = np.full((19, 27), val, np.uint8 if depth == 8 else np.uint16)
            assert np.array_equal(db.deblock_matrix(m, depth, 8, 8, mode), m)
        m = case_plane(np.random.default_rng(depth), 24, 40, depth, above=True)
        for b in (0, 13, 255):          # a = 0: |delta| < 0 never holds; the result is v = min(m, top)
            assert np.array_equal(db.deblock_matrix(m, depth, 8, 8, mode, (0, b)), np.minimum(m, top))
        if depth > 8:
            assert (db.deblock_matrix(np.full((9, 20), 0xFFFF, np.uint16), depth, 8, 8, mode) == top).all()


@pytest.mark.parametrize("mode", MODES)
def test_no_sample_moves_further_than_the_rule_allows(mode):
    """One pass moves no sample by more than (A - 1) // 2; the two together by no more than twice that, and a corner of the grid reaches
    it: four flat blocks of 0, 20 / 20, 40 at a = 25 take the corner sample from 0 to 10 to 20."""
    rng = np.random.default_rng(3)
    for depth in DEPTHS:
        sh = depth - 8
        for a in (1, 2, 25, 100, 255):
            one = ((a << sh) - 1) // 2
            for m in (case_plane(rng, 40, 72, depth), noise_plane(rng, 40, 72, depth)):
                v = m.astype(np.int64)
                only_x = db.deblock_matrix(m[:7], depth, 8, 8, mode, (a, 255)).astype(np.int64)          # 7 rows: no horizontal edge
                only_y = db.deblock_matrix(m[:, :7], depth, 8, 8, mode, (a, 255)).astype(np.int64)          # 7 columns: no vertical edge
                assert np.abs(only_x - v[:7]).max() <= one and np.abs(only_y - v[:, :7]).max() <= one, (depth, a)
                assert np.abs(db.deblock_matrix(m, depth, 8, 8, mode, (a, 255)).astype(np.int64) - v).max() <= 2 * one, (depth, a)
    corner = np.zeros((16, 16), np.uint8)
    corner[:8, 8:] = corner[8:, :8] = 20
    corner[8:, 8:] = 40
    out = db.deblock_matrix(corner, 8, 8, 8, mode, (25, 13))
    assert out[7, 7] == 20 == 2 * ((25 - 1) // 2) - 4 and out[8, 8] == 20


@pytest.mark.parametrize("mode", MODES)
def test_the_sum_is_conserved_where_no_write_is_clamped_or_dropped(mode):
    rng = np.random.default_rng(4)
    seen = 0
    for depth in DEPTHS:
        for block in BLOCKS:
            s = 1 << (depth - 8)
            m = (rng.integers(60, 196, (4 * block, 6 * block)) * s).astype(np.uint16)          # far from 0 and the top: no clamp
            out, counts = db.deblock_matrix(m, depth, block, block, mode, (255, 255), return_counts=True)
            assert counts["clamped"] == 0 and counts["dropped"] == 0 and counts["filtered"] > 0
            assert int(out.sum()) == int(m.sum()) and not np.array_equal(out, m)
            seen += 1
    assert seen == 9
    # a write dropped at the plane's end is not made up for: the edge at the last sample
    m = np.full((1, 9), 100, np.uint8)
    m[0, 8] = 110
    out, counts = db.deblock_matrix(m, 8, 8, 8, mode, (255, 255), return_counts=True)
    assert counts["dropped"] > 0 and int(out.sum()) != int(m.sum())


@pytest.mark.parametrize("mode", MODES)
def test_flips_commute_and_transposition_and_the_pass_order_do_not(mode):
    rng = np.random.default_rng(5)
    for depth in DEPTHS:
        m = case_plane(rng, 40, 72, depth)
        out = db.deblock_matrix(m, depth, 8, 8, mode)
        assert np.array_equal(db.deblock_matrix(m[::-1].copy(), depth, 8, 8, mode), out[::-1])
        assert np.array_equal(db.deblock_matrix(m[:, ::-1].copy(), depth, 8, 8, mode), out[:, ::-1])
        assert not np.array_equal(db.deblock_matrix(m.T.copy(), depth, 8, 8, mode), out.T)
    m = case_plane(np.random.default_rng(7), 40, 72)
    out = db.deblock_matrix(m, 8, 8, 8, mode)
    strong = mode == "strong"
    swapped = db._pass(db._pass(m.astype(np.int64).T, 8, strong, 25, 13, 255, None).T, 8, strong, 25, 13, 255, None)
    assert np.count_nonzero(swapped != out) == {"weak": 170, "strong": 365}[mode]          # pass Y first gives other bytes
    # a dimension that is no multiple of the block: the grid is anchored at the origin, so a flip moves the edges
    odd = case_plane(rng, 40, 70)
    assert not np.array_equal(db.deblock_matrix(odd[:, ::-1].copy(), 8, 8, 8, mode), db.deblock_matrix(odd, 8, 8, 8, mode)[:, ::-1])


def test_a_block_below_8_takes_the_weak_filter():
    rng = np.random.default_rng(6)
    m = case_plane(rng, 24, 40, block=4)
    assert np.array_equal(db.deblock_matrix(m, 8, 4, 4, "strong"), db.deblock_matrix(m, 8, 4, 4, "weak"))
    # per direction: block_y = 4 under strong is strong along the rows and weak down the columns
    x_strong = db._pass(m.astype(np.int64), 8, True, 25, 13, 255, None)
    assert np.array_equal(db.deblock_matrix(m, 8, 4, 8, "strong"), db._pass(x_strong.T, 4, False, 25, 13, 255, None).T.astype(np.uint8))
    assert not np.array_equal(db.deblock_matrix(m, 8, 8, 8, "strong"), db.deblock_matrix(m, 8, 8, 8, "weak"))


# ---------------------------------------------------------------------------------------------------------------------- fields
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("block", BLOCKS)
def test_field_wise_filtering_is_the_two_fields_filtered_by_hand(block, mode):
    rng = np.random.default_rng(block)
    for depth in (8, 10):
        for r in (1, 2, 3, 16, 35):
            m = case_plane(rng, r, 41, depth, above=True, block=block)
            got = db.deblock_fields(m, depth, block, mode)
            want = np.empty_like(m)
            want[0::2] = db.deblock_matrix(m[0::2], depth, block // 2, block, mode)
            if r > 1:
                want[1::2] = db.deblock_matrix(m[1::2], depth, block // 2, block, mode)
            assert np.array_equal(got, want), (depth, r)
            assert np.array_equal(got, db.deblock_plane(m, depth, block, mode, interlaced=True))
            assert np.array_equal(db.deblock_plane(m, depth, block, mode), db.deblock_matrix(m, depth, block, block, mode))
    m = case_plane(rng, 35, 41, block=block)
    assert not np.array_equal(db.deblock_fields(m, 8, block, mode), db.deblock_matrix(m, 8, block, block, mode))


def test_block_4_in_field_mode_leaves_pass_y_out():
    """The fields of block 4 have block_y = 2: a 2-row block has no interior, so the rule is pass X alone, row by row."""
    rng = np.random.default_rng(8)
    m = case_plane(rng, 21, 30, block=4)
    got = db.deblock_fields(m, 8, 4, "strong")
    rows = np.concatenate([db.deblock_matrix(m[y:y + 1], 8, 4, 4, "strong") for y in range(21)])
    assert np.array_equal(got, rows) and np.array_equal(db.deblock_matrix(m, 8, 2, 4, "weak"), rows)
    assert not np.array_equal(got, db.deblock_matrix(m, 8, 4, 4, "strong"))
    with pytest.raises(ValueError, match=r"block_x = 2: 4, 8 or 16"):
        db.deblock_matrix(m, 8, 4, 2)


# ---------------------------------------------------------------------------------------------------------------------- the generator
@pytest.mark.parametrize("mode", MODES)
def test_the_case_generator_takes_every_branch_at_the_defaults(mode):
    """Edges filtered, refused by A, refused by Bt alone, and writes clamped at 0 and at the top: a kernel that never takes one of the
    branches cannot pass on this plane."""
    for depth in DEPTHS:
        m = case_plane(np.random.default_rng(0), *COVER_SHAPE, depth)
        out, counts = db.deblock_matrix(m, depth, 8, 8, mode, return_counts=True)
        assert counts["filtered"] > 50 and counts["refused_a"] > 20 and counts["refused_b"] > 20 and counts["clamped"] >= 2, (depth, counts)
        top = (1 << depth) - 1
        assert out[1, 5:8].tolist() == [top, top, top - 4 * (1 << (depth - 8))] and out[2, 5:8].tolist() == [0, 0, 4 << (depth - 8)]
    m = noise_plane(np.random.default_rng(1), 35, 45)
    _, counts = db.deblock_matrix(m, 8, 8, 8, mode, (255, 255), return_counts=True)
    assert counts["clamped"] > 20 and counts["refused_a"] + counts["refused_b"] < counts["filtered"]
    _, counts = db.deblock_matrix(case_plane(np.random.default_rng(0), 9, 9), 8, 8, 8, mode, (255, 255), return_counts=True)
    assert counts["dropped"] > 0


def test_blocking_falls_on_the_synthetic_picture():
    """A smooth 48 x 64 picture with an offset in -4 .. 4 per 8 x 8 block: the mean squared error against the clean picture falls under
    both modes (measured: 7.37 before, 6.42 after weak, 5.82 after strong)."""
    clean, blocky = blocky_picture()
    mse = lambda a: float(((a.astype(np.float64) - clean) ** 2).mean())          # noqa: E731
    before, weak, strong = mse(blocky), mse(db.deblock_matrix(blocky, mode="weak")), mse(db.deblock_matrix(blocky, mode="strong"))
    print(f"blocky picture: MSE {before:.2f} -> weak {weak:.2f}, strong {strong:.2f}")
    assert weak < before and strong < before


# ---------------------------------------------------------------------------------------------------------------------- frames
def test_deblock_frames_of_every_frame_kind():
    from savsr_amd import yuv
    rng = np.random.default_rng(9)
    v = case_frames(rng, 2, 19, 27, step=3)
    out = db.deblock_frames(v, block=8, mode="strong", interlaced=True)
    for t in range(2):
        for ch in range(3):
            assert np.array_equal(out[t, :, :, ch], db.deblock_fields(v[t, :, :, ch], 8, 8, "strong"))
    assert np.array_equal(db.deblock_frames(torch.from_numpy(v)), db.deblock_frames(v))
    for fmt, layout, depth, (h, w) in (("i420", "420", 8, (19, 37)), ("i422", "422", 10, (18, 36)), ("i444", "444", 12, (17, 18)), ("y400", "400", 8, (9, 33))):
        sizes = [(h, w)] + ([] if layout == "400" else [yuv.chroma_hw(h, w, layout)] * 2)
        planes = [case_frames(rng, 2, *hw, depth=depth) for hw in sizes]
        frames = np.ascontiguousarray(np.concatenate([as_bytes(p) for p in planes], 1))
        got = db.deblock_frames(frames, fmt, (h, w), depth, 8, "weak", (25, 13), (60, 30))
        want = np.concatenate([as_bytes(np.stack([db.deblock_matrix(p[t, :, :, 0], depth, 8, 8, "weak", (25, 13) if i == 0 else (60, 30)) for t in range(2)]))
                               for i, p in enumerate(planes)], 1)
        assert got.dtype == np.uint8 and np.array_equal(got, want), fmt
    with pytest.raises(ValueError, match="float frames have no integer samples to deblock"):
        db.deblock_frames(np.zeros((2, 8, 8, 3), np.float32))
    with pytest.raises(ValueError, match=r"frames of 8 x 8 are \[N, 96\] uint8"):
        db.deblock_frames(np.zeros((2, 95), np.uint8), "i420", (8, 8))
    with pytest.raises(ValueError, match="depth = 10 goes with pixel_format"):
        db.deblock_frames(np.zeros((2, 8, 8, 3), np.uint8), depth=10)


# ---------------------------------------------------------------------------------------------------------------------- the refusals
def test_option_checks_and_their_wording():
    assert (db.DEBLOCKERS, db.DEFAULT_BLOCK, db.DEFAULT_STRENGTH) == (("weak", "strong"), 8, (25, 13))
    assert db.DEFAULT_STRENGTH == (int(round(0.098 * 255)), int(round(0.05 * 255)))          # ffmpeg deblock's alpha / beta in codes
    assert db.check_deblock_options(None, 8, (25, 13), None) is None and db.check_deblock_options(None, 8, [25, 13], None) is None
    assert db.check_deblock_options("weak", 8, (25, 13), None) == (8, "weak", (25, 13), (25, 13))
    assert db.check_deblock_options("strong", 16, [0, 255], (1, 2)) == (16, "strong", (0, 255), (1, 2))
    for args, words in ((("medium", 8, (25, 13), None), r"deblock = 'medium': None or one of weak, strong"),
                        ((True, 8, (25, 13), None), r"deblock = True: None or one of weak, strong"),
                        ((None, 4, (25, 13), None), r"deblock_block = 4 goes with deblock=: without the stage there is nothing to set"),
                        ((None, 8, (25, 12), None), r"deblock_strength = \(25, 12\) goes with deblock="),
                        ((None, 8, (25, 13), (25, 13)), r"deblock_chroma_strength = \(25, 13\) goes with deblock="),
                        (("weak", 12, (25, 13), None), r"deblock_block = 12: 4, 8 or 16"),
                        (("weak", 8.0, (25, 13), None), r"deblock_block = 8\.0: 4, 8 or 16"),
                        (("weak", True, (25, 13), None), r"deblock_block = True: 4, 8 or 16"),
                        (("weak", 8, (25, 256), None), r"deblock_strength = \(25, 256\): two ints \(a, b\) in 0 \.\. 255"),
                        (("weak", 8, (-1, 13), None), r"deblock_strength = \(-1, 13\): two ints"),
                        (("weak", 8, (25.0, 13), None), r"deblock_strength = \(25\.0, 13\): two ints"),
                        (("weak", 8, (25, 13, 1), None), r"deblock_strength = \(25, 13, 1\): two ints"),
                        (("weak", 8, 25, None), r"deblock_strength = 25: two ints"),
                        (("weak", 8, (True, 13), None), r"deblock_strength = \(True, 13\): two ints"),
                        (("weak", 8, (25, 13), (300, 1)), r"deblock_chroma_strength = \(300, 1\): two ints")):
        with pytest.raises(ValueError, match=words):
            db.check_deblock_options(*args)
    with pytest.raises(ValueError, match=r"--deblock-block = 5: 4, 8 or 16"):
        db.check_deblock_options("weak", 5, (25, 13), None, prefix="--deblock-")
    m = np.zeros((4, 4), np.uint8)
    for kw, words in ((dict(mode="medium"), r"mode = 'medium': one of weak, strong"), (dict(thr=(1, 2, 3)), r"thr = \(1, 2, 3\): two ints"),
                      (dict(block_y=3), r"block_y = 3: 2 \(the fields of block 4: no pass Y\), 4, 8 or 16"), (dict(block_x=32), r"block_x = 32: 4, 8 or 16"),
                      (dict(depth=9), r"depth = 9: 8, 10 or 12")):
        with pytest.raises(ValueError, match=words):
            db.deblock_matrix(m, **kw)
    with pytest.raises(ValueError, match=r"must be \[R, C\] integers"):
        db.deblock_matrix(np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError, match=r"must be \[R, C\] integers"):
        db.deblock_fields(np.zeros((2, 2, 2), np.uint8))
    with pytest.raises(ValueError, match=r"a matrix of 0 x 4"):
        db.deblock_matrix(np.zeros((0, 4), np.uint8))
    with pytest.raises(ValueError, match=r"block = 2: 4, 8 or 16"):
        db.deblock_fields(m, 8, 2)


def test_the_video_calls_refuse_before_the_gpu_is_touched():
    """upscale_video / VideoUpscaler on a network that is not on a GPU: every refusal below is raised on the host, before the call would
    have asked for the device (a good call ends at that question)."""
    from savsr_amd import VideoUpscaler
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR(num_feat=32).eval()
    v = torch.zeros(8, 12, 16, 3, dtype=torch.uint8)
    calls = (lambda **kw: net.upscale_video(v, scale=2, out="uint8", **kw), lambda **kw: VideoUpscaler(net, 2, out="uint8", **kw))
    for call in calls:
        for kw, words in ((dict(deblock="medium"), r"deblock = 'medium': None or one of weak, strong"),
                          (dict(deblock=1), r"deblock = 1: None or one of weak, strong"),
                          (dict(deblock_block=16), r"deblock_block = 16 goes with deblock="),
                          (dict(deblock_strength=(4, 9)), r"deblock_strength = \(4, 9\) goes with deblock="),
                          (dict(deblock_chroma_strength=(4, 9)), r"deblock_chroma_strength = \(4, 9\) goes with deblock="),
                          (dict(deblock="weak", deblock_block=2), r"deblock_block = 2: 4, 8 or 16"),
                          (dict(deblock="strong", deblock_strength=(256, 0)), r"deblock_strength = \(256, 0\): two ints \(a, b\) in 0 \.\. 255"),
                          (dict(deblock="strong", deblock_strength=3.0), r"deblock_strength = 3\.0: two ints"),
                          (dict(deblock="strong", deblock_chroma_strength=(1,)), r"deblock_chroma_strength = \(1,\): two ints")):
            with pytest.raises(ValueError, match=words):
                call(**kw)
    with pytest.raises(TypeError):                                                   # keyword only
        net.upscale_video(v, 2, "reflection", "uint8", "rgb", None, None, 10.0, "bt601", None, 8, None, None, None, None, None, 24, "keep", None, None, 5,
                          "weak")
    f = torch.zeros(8, 3, 12, 16)
    with pytest.raises(ValueError, match="float frames"):          # (host floats are refused as such; floats on the GPU by the stage: the GPU tests)
        net.upscale_video(f, scale=2, deblock="weak")
    with pytest.raises(ValueError, match="float frames have no integer samples to deblock"):
        VideoUpscaler(net, 2, deblock="weak").push(f)
    with pytest.raises(RuntimeError, match="AMD GPU only"):                          # a good call gets as far as the device
        net.upscale_video(v, scale=2, out="uint8", deblock="strong", deblock_block=16, deblock_strength=(255, 0), deblock_chroma_strength=(0, 0))
    with pytest.raises(ValueError, match="float frames have no integer samples to deblock"):
        savsr_amd.deblock_video(f)
    with pytest.raises(ValueError, match=r"block = 5: 4, 8 or 16"):
        savsr_amd.deblock_video(v, block=5)
    with pytest.raises(ValueError, match=r"mode = 'none': one of weak, strong"):
        savsr_amd.deblock_video(v, mode="none")
    with pytest.raises(ValueError, match=r"chroma_strength = \(1, 999\)"):
        savsr_amd.deblock_video(v, chroma_strength=(1, 999))


def test_the_stage_in_video_upscaler_is_stateless():
    """deblock= builds no streaming stage (nothing that holds frames back), only the checked options that push() applies to the chunk it
    was given; it is field-wise exactly with fields= or pulldown=."""
    from savsr_amd import VideoUpscaler
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR(num_feat=32).eval()
    up = VideoUpscaler(net, 2, out="uint8", deblock="strong", deblock_block=16, deblock_chroma_strength=(1, 2))
    assert up._edges == (16, "strong", (25, 13), (1, 2)) and not up._fieldwise and up._noise is None and up._split is None and up._buf is None
    plain = VideoUpscaler(net, 2, out="uint8")
    assert plain._edges is None
    assert VideoUpscaler(net, 2, out="uint8", deblock="weak", fields="bff")._fieldwise
    assert VideoUpscaler(net, 2, out="uint8", deblock="weak", pulldown="tff")._fieldwise


# ---------------------------------------------------------------------------------------------------------------------- the CLI
def test_cli_arguments(capsys):
    from savsr_amd.upscale import deblock_kwargs, parse_args
    base = ["-i", "in.y4m", "-o", "out.y4m", "--scale", "2", "--checkpoint", "x.pth"]
    a = parse_args(base)
    assert a.deblock is None and deblock_kwargs(a) == {}
    assert deblock_kwargs(parse_args(base + ["--deblock", "none"])) == {}
    a = parse_args(base + ["--deblock", "weak"])
    assert deblock_kwargs(a) == dict(deblock="weak", deblock_block=8, deblock_strength=(25, 13), deblock_chroma_strength=None)
    a = parse_args(base + ["--deblock", "strong", "--deblock-block", "16", "--deblock-strength", "40, 20", "--deblock-chroma-strength", "60,30"])
    assert deblock_kwargs(a) == dict(deblock="strong", deblock_block=16, deblock_strength=(40, 20), deblock_chroma_strength=(60, 30))
    png = ["-i", "in", "-o", "out", "--scale", "2", "--checkpoint", "x.pth"]
    assert deblock_kwargs(parse_args(png + ["--deblock", "strong", "--deblock-block", "4"]))["deblock_block"] == 4
    a = parse_args(base + ["--denoise", "ata", "--spatial-denoise", "nlm", "--deblock", "weak", "--scan", "detect"])          # the stages go together
    assert a.denoise == "ata" and a.spatial_denoise == "nlm" and a.deblock == "weak"
    for extra, words in ((["--deblock-block", "8"], "go with --deblock weak or strong"),
                         (["--deblock-strength", "25,13"], "go with --deblock weak or strong"),
                         (["--deblock", "none", "--deblock-chroma-strength", "1,1"], "go with --deblock weak or strong"),
                         (["--deblock", "weak", "--deblock-block", "12"], "--deblock-block = 12: 4, 8 or 16"),
                         (["--deblock", "weak", "--deblock-block", "x"], "invalid int value"),
                         (["--deblock", "weak", "--deblock-strength", "25"], "--deblock-strength: A,B, got '25'"),
                         (["--deblock", "weak", "--deblock-strength", "a,b"], "--deblock-strength: A,B with integers"),
                         (["--deblock", "weak", "--deblock-strength", "25,256"], "--deblock-strength = (25, 256): two ints (a, b) in 0 .. 255"),
                         (["--deblock", "strong", "--deblock-chroma-strength", "300,3"], "--deblock-chroma-strength = (300, 3)"),
                         (["--deblock", "medium"], "invalid choice")):
        with pytest.raises(SystemExit):
            parse_args(base + extra)
        assert words in capsys.readouterr().err, extra
    with pytest.raises(SystemExit):
        parse_args(png + ["--deblock", "weak", "--deblock-chroma-strength", "2,2"])
    assert "goes with a Y4M input" in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------------------------------- the ABI
def test_header_binding_and_library_agree_at_abi_52():
    hdr = open(os.path.join(ROOT, "include", "savsr_hip.h")).read()
    assert int(re.search(r"#define\s+SAVSR_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 52
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    assert lib.savsr_abi_version() == _lib.ABI_VERSION
    for name in ("savsr_video_deblock_u8", "savsr_video_deblock_u16"):
        decl = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, plain, flags=re.S)
        assert decl, name
        params = [p.strip() for p in decl.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert len(params) == len(args), (name, params)
        for p, t in zip(params, args):          # pointers travel as void pointers, int64_t as c_int64, int as c_int
            want = _lib.C.c_void_p if "*" in p else _lib.C.c_int64 if p.startswith("int64_t") else _lib.C.c_int
            assert t is want, (name, p)
        assert hasattr(lib, name)
    names = [p.split()[-1].lstrip("*") for p in re.search(r"savsr_video_deblock_u16\s*\((.*?)\);", plain, flags=re.S).group(1).split(",")]
    assert names == ["frames", "n_frames", "frame_bytes", "plane_offset", "rows", "cols", "step", "depth", "block", "strong", "interlaced", "thr_a",
                     "thr_b", "out", "out_frame_bytes", "out_plane_offset", "stream"]
    build = open(os.path.join(ROOT, "savsr_amd", "csrc", "build.sh")).read()
    assert build.count("deblock.hip") == 2
    assert callable(savsr_amd.deblock_video) and savsr_amd.deblock is db
    # the entries refuse on the host, by name, before the device is touched
    assert lib.savsr_video_deblock_u8(0, 1, 1, 0, 1, 1, 1, 8, 0, 0, 25, 13, 0, 1, 0, None) == -1
    assert b"video_deblock_u8: null pointer" in lib.savsr_last_error()
    buf = (_lib.C.c_uint8 * 256)()
    p = _lib.C.addressof(buf)
    for args, words in (((p, 1, 64, 0, 8, 8, 1, 5, 0, 0, 25, 13, p + 128, 64, 0), b"video_deblock_u8: block 4, 8 or 16"),
                        ((p, 1, 64, 0, 8, 8, 1, 8, 0, 0, 256, 13, p + 128, 64, 0), b"video_deblock_u8: thresholds 0 .. 255 << (depth - 8)"),
                        ((p, 1, 64, 0, 8, 8, 1, 8, 0, 0, 25, 13, p + 32, 64, 0), b"video_deblock_u8: the source frames and the output overlap")):
        assert lib.savsr_video_deblock_u8(*args, None) == -1 and words in lib.savsr_last_error(), args


# ---------------------------------------------------------------------------------------------------------------------- the host check
CXX = os.environ.get("CXX") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++"))


@pytest.mark.skipif(not CXX, reason="no clang++: the sanitizer build of the kernels' code needs one")
def test_the_kernels_code_passes_the_sanitizer_host_check():
    """tools/check_deblock_host.py: csrc/deblock.hip's entries and the four phases of its kernel as a stand-alone host program under
    ASan / UBSan, against the specification (the tool's docstring says what the host form covers and what only the GPU tests do)."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_deblock_host.py"), "--cxx", CXX], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "cases equal the specification or are refused by name, no sanitizer report" in res.stdout
