"""CPU checks of the deringing stage's specification (savsr_amd/dering.py): the vectorised rule against a slow restatement block by block
and sample by sample, the properties that follow from the rule, the tie rule, both tap sets and both variance branches, the ringing
picture, field-wise filtering, depths, frames of every kind, the option checks, the video calls' refusals before the GPU is touched, the
command line's arguments, the C surface, and the sanitizer host check of the kernels' code."""
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
from savsr_amd import dering as dr
from tests.dering_cases import DEPTHS, STRENGTHS, TIE_SHAPE, as_bytes, case_frames, case_plane, constant_blocks, noise_plane, ringing_picture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------- the slow restatement
def _msb(n):
    return n.bit_length() - 1


def _con(delta, T, q):
    a = abs(delta)
    m = min(a, max(0, T - (a >> q)))
    return -m if delta < 0 else m


def slow_dering(m, depth=8, strength=(4, 2), damping=5, tie=None):
    """The rule of the module's docstring, written again without numpy's help: a Python loop per block and per sample, Python ints.
    tie: the direction a block of eight equal costs takes (None: the rule's, the smallest index); returns (result, directions, P8s)."""
    p, s = strength
    R, C = m.shape
    sh, top = depth - 8, (1 << depth) - 1
    v = [[min(int(x), top) for x in row] for row in m]
    at = lambda y, x: v[min(max(y, 0), R - 1)][min(max(x, 0), C - 1)]          # noqa: E731
    W = [0, 840, 420, 280, 210, 168, 140, 120, 105]
    dirs_tab = [[(-1, 1), (-2, 2)], [(0, 1), (-1, 2)], [(0, 1), (0, 2)], [(0, 1), (1, 2)], [(1, 1), (2, 2)], [(1, 0), (2, 1)], [(1, 0), (2, 0)],
                [(1, 0), (2, -1)]]
    out = np.array(v, dtype=np.int64)
    seen_dir, seen_p8 = {}, {}
    for by in range(-(-R // 8)):
        for bx in range(-(-C // 8)):
            part = [[0] * 15 for _ in range(8)]
            for i in range(8):
                for j in range(8):
                    b = (at(8 * by + i, 8 * bx + j) >> sh) - 128
                    for k, n in enumerate((i + j, i + j // 2, i, 3 + i - j // 2, 7 + i - j, 3 - i // 2 + j, j, i // 2 + j)):
                        part[k][n] += b
            cost = [0] * 8
            for k in (2, 6):
                cost[k] = 105 * sum(part[k][i] ** 2 for i in range(8))
            for k in (0, 4):
                cost[k] = sum((part[k][i] ** 2 + part[k][14 - i] ** 2) * W[i + 1] for i in range(7)) + 105 * part[k][7] ** 2
            for k in (1, 3, 5, 7):
                cost[k] = 105 * sum(part[k][3 + j] ** 2 for j in range(5)) + sum((part[k][j] ** 2 + part[k][10 - j] ** 2) * W[2 * j + 2] for j in range(3))
            assert max(cost) <= 880803840
            d = cost.index(max(cost))
            if tie is not None and len(set(cost)) == 1:
                d = tie
            var = (cost[d] - cost[(d + 4) & 7]) >> 10
            P8 = 0 if var == 0 else (p * (4 + (0 if var < 64 else min(_msb(var >> 6), 12))) + 8) >> 4
            seen_dir[by, bx], seen_p8[by, bx] = d, P8
            P, S, Dd = P8 << sh, s << sh, damping + sh
            for y in range(8 * by, min(8 * by + 8, R)):
                for c in range(8 * bx, min(8 * bx + 8, C)):
                    x = v[y][c]
                    total, lo, hi = 0, x, x
                    classes = []
                    if P > 0:
                        classes.append((dirs_tab[d], (3, 3) if P8 & 1 else (4, 2), P, max(0, Dd - _msb(P))))
                    if S > 0:
                        classes.append((dirs_tab[(d + 2) & 7], (2, 1), S, max(0, Dd - _msb(S))))
                        classes.append((dirs_tab[(d + 6) & 7], (2, 1), S, max(0, Dd - _msb(S))))
                    for taps, w, T, q in classes:
                        for k in (0, 1):
                            for sign in (1, -1):
                                t = at(y + sign * taps[k][0], c + sign * taps[k][1])
                                total += w[k] * _con(t - x, T, q)
                                lo, hi = min(lo, t), max(hi, t)
                    out[y, c] = min(max(x + ((8 + total - (1 if total < 0 else 0)) >> 4), lo), hi)
    return out.astype(m.dtype), seen_dir, seen_p8


# ---------------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("depth", DEPTHS)
def test_the_vectorised_rule_is_the_slow_one(depth):
    rng = np.random.default_rng(depth)
    for strength, damping, shape, kind in (((4, 2), 5, (27, 35), "case"), ((15, 4), 3, (17, 22), "noise"), ((7, 0), 6, (9, 9), "case"),
                                           ((0, 3), 4, (20, 13), "case"), ((4, 2), 5, (1, 1), "noise"), ((4, 2), 5, (1, 9), "noise")):
        m = noise_plane(rng, *shape, depth) if kind == "noise" else case_plane(rng, *shape, depth, above=True)
        want, dirs, p8 = slow_dering(m, depth, strength, damping)
        assert np.array_equal(dr.dering_matrix(m, depth, strength, damping), want), (depth, strength, damping, shape)
        d_b, var_b = dr.block_directions(np.minimum(m.astype(np.int64), (1 << depth) - 1), depth)
        assert all(d_b[k] == v for k, v in dirs.items()) and all(dr.primary8(var_b, strength[0])[k] == v for k, v in p8.items())


def test_the_cost_bound_is_reached_by_a_block_of_zeros():
    d, var = dr.block_directions(np.zeros((8, 8), np.int64))
    assert d[0, 0] == 0 and var[0, 0] == 0          # a constant block: eight equal costs
    # each of the eight costs of b = -128 everywhere is 880 803 840 (slow_dering asserts the bound on every block it sees)
    assert 105 * 8 * (8 * 128) ** 2 == 880803840 < 2 ** 31


@pytest.mark.parametrize("strength", STRENGTHS)
def test_constant_planes_and_the_zero_strength(strength):
    for depth in DEPTHS:
        c = np.full((19, 21), 77 << (depth - 8), np.uint8 if depth == 8 else np.uint16)
        assert np.array_equal(dr.dering_matrix(c, depth, strength), c)
        assert np.array_equal(dr.dering_fields(c, depth, strength), c)
    m = case_plane(np.random.default_rng(1), 37, 41, 10, above=True)
    assert (m > 1023).any()
    if strength == (0, 0):
        assert np.array_equal(dr.dering_matrix(m, 10, strength), np.minimum(m, 1023))          # the identity on v
    else:
        assert not np.array_equal(dr.dering_matrix(m, 10, strength), np.minimum(m, 1023))


@pytest.mark.parametrize("depth", DEPTHS)
def test_outputs_stay_within_their_taps_and_move_no_further_than_the_rule_allows(depth):
    rng = np.random.default_rng(10 + depth)
    sh, top = depth - 8, (1 << depth) - 1
    for m in (case_plane(rng, 40, 53, depth, above=True), noise_plane(rng, 33, 29, depth)):
        v = np.minimum(m.astype(np.int64), top)
        vp = np.pad(v, 2, mode="edge")
        near = np.stack([vp[2 + dy:2 + dy + v.shape[0], 2 + dx:2 + dx + v.shape[1]] for dy in range(-2, 3) for dx in range(-2, 3)])
        for p, s in STRENGTHS + ((15, 0), (1, 1)):
            for damping in (3, 6):
                got = dr.dering_matrix(m, depth, (p, s), damping).astype(np.int64)
                assert (got >= near.min(0)).all() and (got <= near.max(0)).all()          # (every tap lies within the 5 x 5 neighbourhood)
                P8 = np.repeat(np.repeat(dr.primary8(dr.block_directions(v, depth)[1], p), 8, 0), 8, 1)[:v.shape[0], :v.shape[1]]
                assert P8.max() <= 15
                assert (np.abs(got - v) <= (12 * ((P8 << sh) + (s << sh)) + 8) >> 4).all(), (depth, p, s, damping)


def test_a_split_at_a_multiple_of_8_changes_only_samples_within_2_of_the_cut():
    rng = np.random.default_rng(3)
    m = case_plane(rng, 40, 56)
    whole = dr.dering_matrix(m, 8, (15, 4))
    for cut in (8, 24):
        parts = np.concatenate([dr.dering_matrix(m[:cut], 8, (15, 4)), dr.dering_matrix(m[cut:], 8, (15, 4))], 0)
        diff = np.argwhere(parts != whole)
        assert len(diff) and ((diff[:, 0] >= cut - 2) & (diff[:, 0] < cut + 2)).all(), cut
        parts = np.concatenate([dr.dering_matrix(m[:, :cut], 8, (15, 4)), dr.dering_matrix(m[:, cut:], 8, (15, 4))], 1)
        diff = np.argwhere(parts != whole)
        assert len(diff) and ((diff[:, 1] >= cut - 2) & (diff[:, 1] < cut + 2)).all(), cut


def test_the_tie_rule_the_smallest_index_wins():
    """A plane of constant 8 x 8 blocks: every block has eight equal costs, var = 0 and P8 = 0, so only the secondary taps act, along
    directions (dir + 2) & 7 and (dir + 6) & 7 -- 2 and 6 for dir = 0, across the block borders.  The independent restatement pins
    direction 0; had constant blocks taken direction 7 (the last index), other samples would change."""
    m = constant_blocks(*TIE_SHAPE)
    assert m.min() >= 100 and m.max() <= 139
    got, counts = dr.dering_matrix(m, return_counts=True)
    want, dirs, p8 = slow_dering(m)
    assert np.array_equal(got, want) and set(dirs.values()) == {0} and set(p8.values()) == {0}
    assert counts["flat"] == 45 and counts["changed"] == np.count_nonzero(got != m) > 0
    last, dirs7, _ = slow_dering(m, tie=7)
    assert set(dirs7.values()) == {7} and np.count_nonzero(last != got) > 0


def test_both_tap_sets_and_both_variance_branches_occur():
    m = case_plane(np.random.default_rng(5), 48, 96)
    _, counts = dr.dering_matrix(m, 8, (4, 2), return_counts=True)
    assert counts["even_taps"] > 0 and counts["odd_taps"] > 0, counts          # (4, 2) and (3, 3)
    assert counts["var_low"] > 0 and counts["var_high"] > 0 and counts["flat"] > 0, counts
    d_b, _ = dr.block_directions(m.astype(np.int64))
    assert len(set(d_b.ravel().tolist())) >= 5          # several directions win


def test_ringing_falls_on_the_dct_quantised_picture():
    clean, coded = ringing_picture()
    before = np.mean((coded - clean) ** 2)
    after = np.mean((dr.dering_matrix(coded) - clean) ** 2)
    assert after < before, (before, after)


def test_field_wise_filtering_is_the_two_fields_filtered_by_hand():
    rng = np.random.default_rng(6)
    for rows in (1, 2, 17, 35):
        m = case_plane(rng, rows, 29) if rows > 2 else noise_plane(rng, rows, 29)
        got = dr.dering_fields(m, 8, (15, 4))
        assert np.array_equal(got[0::2], dr.dering_matrix(m[0::2], 8, (15, 4)))
        if rows > 1:
            assert np.array_equal(got[1::2], dr.dering_matrix(m[1::2], 8, (15, 4)))
        assert np.array_equal(dr.dering_plane(m, 8, (15, 4), 5, True), got)
    m = case_plane(rng, 35, 29)
    assert not np.array_equal(dr.dering_fields(m), dr.dering_matrix(m))          # field-wise is another filter
    assert np.array_equal(dr.dering_plane(m), dr.dering_matrix(m))


@pytest.mark.parametrize("depth", (10, 12))
def test_depths_scale_strength_and_damping_and_read_samples_above_the_range_as_the_top(depth):
    rng = np.random.default_rng(depth)
    m8 = case_plane(rng, 24, 40)
    sh = depth - 8
    # an 8-bit plane shifted up has the directions and the 8-bit primary strengths of the 8-bit plane: step 1 reads v >> sh
    d8, var8 = dr.block_directions(m8.astype(np.int64), 8)
    d, var = dr.block_directions(m8.astype(np.int64) << sh, depth)
    assert np.array_equal(d, d8) and np.array_equal(var, var8)
    # and strengths in the depth's codes: no sample moves further than the 8-bit bound shifted up
    up = m8.astype(np.uint16) << sh
    moved = np.abs(dr.dering_matrix(up, depth, (9, 3), 4).astype(np.int64) - up)
    assert 0 < moved.max() <= (12 * ((15 << sh) + (3 << sh)) + 8) >> 4
    m = case_plane(rng, 24, 40, depth, above=True)
    assert (m > (1 << depth) - 1).any()
    got = dr.dering_matrix(m, depth)
    assert got.dtype == np.uint16 and got.max() <= (1 << depth) - 1
    assert np.array_equal(got, dr.dering_matrix(np.minimum(m, (1 << depth) - 1), depth))


def test_dering_frames_of_every_frame_kind():
    from savsr_amd import yuv
    rng = np.random.default_rng(8)
    v = case_frames(rng, 2, 19, 27, step=3)
    got = dr.dering_frames(v)
    for t in range(2):
        for ch in range(3):
            assert np.array_equal(got[t, :, :, ch], dr.dering_matrix(v[t, :, :, ch]))
    assert np.array_equal(dr.dering_frames(torch.from_numpy(v), interlaced=True)[1, :, :, 2], dr.dering_fields(v[1, :, :, 2]))
    for fmt, layout, depth, (h, w) in (("i420", "420", 8, (18, 36)), ("i422", "422", 10, (18, 36)), ("i444", "444", 12, (9, 18)), ("y400", "400", 8, (9, 33))):
        sizes = [(h, w)] + ([] if layout == "400" else [yuv.chroma_hw(h, w, layout)] * 2)
        planes = [case_frames(rng, 2, *hw, depth=depth) for hw in sizes]
        frames = np.ascontiguousarray(np.concatenate([as_bytes(p) for p in planes], 1))
        got = dr.dering_frames(frames, fmt, (h, w), depth, (4, 2), (15, 4), 5, True)
        want = np.concatenate([as_bytes(np.stack([dr.dering_fields(p[t, :, :, 0], depth, (4, 2) if i == 0 else (15, 4)) for t in range(2)])[..., None])
                               for i, p in enumerate(planes)], 1)
        assert np.array_equal(got, want), fmt
    with pytest.raises(ValueError, match="float frames have no integer samples to dering"):
        dr.dering_frames(np.zeros((1, 4, 4, 3), np.float32))
    with pytest.raises(ValueError, match="packed frames are 8-bit"):
        dr.dering_frames(v, depth=10)


# ---------------------------------------------------------------------------------------------------------------------- options
def test_option_checks_and_their_wording():
    assert dr.DERINGERS == ("cdef",) and dr.DEFAULT_STRENGTH == (4, 2) and dr.DEFAULT_DAMPING == 5
    assert "nothing is validated on footage" in dr.__doc__ and "nothing here is pinned to libaom's or ffmpeg's output" in dr.__doc__
    assert dr.check_dering_options(None, (4, 2), None, 5) is None
    assert dr.check_dering_options("cdef", (4, 2), None, 5) == ((4, 2), (4, 2), 5)
    assert dr.check_dering_options("cdef", [15, 0], (0, 4), 3) == ((15, 0), (0, 4), 3)
    for args, words in ((("CDEF", (4, 2), None, 5), r"dering = 'CDEF': None or one of cdef"),
                        ((1, (4, 2), None, 5), r"dering = 1: None or one of cdef"),
                        ((None, (4, 3), None, 5), r"dering_strength = \(4, 3\) goes with dering="),
                        ((None, (4, 2), (4, 2), 5), r"dering_chroma_strength = \(4, 2\) goes with dering="),
                        ((None, (4, 2), None, 6), r"dering_damping = 6 goes with dering="),
                        (("cdef", (16, 2), None, 5), r"dering_strength = \(16, 2\): two ints \(p, s\), 0 <= p <= 15 and 0 <= s <= 4"),
                        (("cdef", (4, 5), None, 5), r"dering_strength = \(4, 5\): two ints"),
                        (("cdef", (4, -1), None, 5), r"dering_strength = \(4, -1\): two ints"),
                        (("cdef", (4.0, 2), None, 5), r"dering_strength = \(4\.0, 2\): two ints"),
                        (("cdef", (True, 2), None, 5), r"dering_strength = \(True, 2\): two ints"),
                        (("cdef", 4, None, 5), r"dering_strength = 4: two ints"),
                        (("cdef", (4, 2), (1,), 5), r"dering_chroma_strength = \(1,\): two ints"),
                        (("cdef", (4, 2), None, 2), r"dering_damping = 2: an int in 3 \.\. 6"),
                        (("cdef", (4, 2), None, 7), r"dering_damping = 7: an int in 3 \.\. 6"),
                        (("cdef", (4, 2), None, 5.0), r"dering_damping = 5\.0: an int in 3 \.\. 6")):
        with pytest.raises(ValueError, match=words):
            dr.check_dering_options(*args)
    m = np.zeros((4, 4), np.uint8)
    with pytest.raises(ValueError, match=r"depth = 9: 8, 10 or 12"):
        dr.dering_matrix(m, 9)
    with pytest.raises(ValueError, match=r"the matrix must be \[R, C\] integers"):
        dr.dering_matrix(m.astype(np.float32))
    with pytest.raises(ValueError, match=r"a matrix of 0 x 4"):
        dr.dering_matrix(np.zeros((0, 4), np.uint8))
    with pytest.raises(ValueError, match=r"strength = \(4, 9\)"):
        dr.dering_fields(m, 8, (4, 9))


def test_the_video_calls_refuse_before_the_gpu_is_touched():
    """upscale_video / VideoUpscaler on a network that is not on a GPU: every refusal below is raised on the host, before the call would
    have asked for the device (a good call ends at that question)."""
    from savsr_amd import VideoUpscaler
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR(num_feat=32).eval()
    v = torch.zeros(8, 12, 16, 3, dtype=torch.uint8)
    calls = (lambda **kw: net.upscale_video(v, scale=2, out="uint8", **kw), lambda **kw: VideoUpscaler(net, 2, out="uint8", **kw))
    for call in calls:
        for kw, words in ((dict(dering="strong"), r"dering = 'strong': None or one of cdef"),
                          (dict(dering_strength=(4, 3)), r"dering_strength = \(4, 3\) goes with dering="),
                          (dict(dering_chroma_strength=(4, 2)), r"dering_chroma_strength = \(4, 2\) goes with dering="),
                          (dict(dering_damping=3), r"dering_damping = 3 goes with dering="),
                          (dict(dering="cdef", dering_strength=(16, 0)), r"dering_strength = \(16, 0\): two ints"),
                          (dict(dering="cdef", dering_chroma_strength=(1,)), r"dering_chroma_strength = \(1,\): two ints"),
                          (dict(dering="cdef", dering_damping=7), r"dering_damping = 7: an int in 3 \.\. 6")):
            with pytest.raises(ValueError, match=words):
                call(**kw)
    f = torch.zeros(8, 3, 12, 16)
    with pytest.raises(ValueError, match="float frames"):          # (host floats are refused as such; floats on the GPU by the stage: the GPU tests)
        net.upscale_video(f, scale=2, dering="cdef")
    with pytest.raises(ValueError, match="float frames have no integer samples to dering"):
        VideoUpscaler(net, 2, dering="cdef").push(f)
    with pytest.raises(RuntimeError, match="AMD GPU only"):                          # a good call gets as far as the device
        net.upscale_video(v, scale=2, out="uint8", dering="cdef", dering_strength=(15, 4), dering_chroma_strength=(0, 0), dering_damping=6)
    with pytest.raises(RuntimeError, match="AMD GPU only"):                          # beside the deblocker
        net.upscale_video(v, scale=2, out="uint8", deblock="strong", dering="cdef")
    with pytest.raises(ValueError, match="float frames have no integer samples to dering"):
        savsr_amd.dering_video(f)
    with pytest.raises(ValueError, match=r"strength = \(99, 0\)"):
        savsr_amd.dering_video(v, strength=(99, 0))
    with pytest.raises(ValueError, match=r"chroma_strength = \(1, 999\)"):
        savsr_amd.dering_video(v, chroma_strength=(1, 999))
    with pytest.raises(ValueError, match=r"damping = 9"):
        savsr_amd.dering_video(v, damping=9)


def test_the_stage_in_video_upscaler_is_stateless():
    """dering= builds no streaming stage (nothing that holds frames back), only the checked options that push() applies to the chunk it
    was given; it is field-wise exactly with fields= or pulldown=, as the deblocker is."""
    from savsr_amd import VideoUpscaler
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR(num_feat=32).eval()
    up = VideoUpscaler(net, 2, out="uint8", dering="cdef", dering_chroma_strength=(1, 2), dering_damping=3)
    assert up._rings == ((4, 2), (1, 2), 3) and not up._fieldwise and up._edges is None and up._noise is None and up._split is None and up._buf is None
    assert VideoUpscaler(net, 2, out="uint8")._rings is None
    assert VideoUpscaler(net, 2, out="uint8", dering="cdef", fields="bff")._fieldwise
    assert VideoUpscaler(net, 2, out="uint8", dering="cdef", pulldown="tff")._fieldwise


# ---------------------------------------------------------------------------------------------------------------------- the CLI
def test_cli_arguments(capsys):
    from savsr_amd.upscale import dering_kwargs, parse_args
    base = ["-i", "in.y4m", "-o", "out.y4m", "--scale", "2", "--checkpoint", "x.pth"]
    a = parse_args(base)
    assert a.dering is None and dering_kwargs(a) == {}
    assert dering_kwargs(parse_args(base + ["--dering", "none"])) == {}
    assert dering_kwargs(parse_args(base + ["--dering", "cdef"])) == dict(dering="cdef", dering_strength=(4, 2), dering_chroma_strength=None, dering_damping=5)
    a = parse_args(base + ["--dering", "cdef", "--dering-strength", "9, 3", "--dering-chroma-strength", "15,4", "--dering-damping", "6"])
    assert dering_kwargs(a) == dict(dering="cdef", dering_strength=(9, 3), dering_chroma_strength=(15, 4), dering_damping=6)
    png = ["-i", "in", "-o", "out", "--scale", "2", "--checkpoint", "x.pth"]
    assert dering_kwargs(parse_args(png + ["--dering", "cdef", "--dering-damping", "3"]))["dering_damping"] == 3
    a = parse_args(base + ["--denoise", "ata", "--spatial-denoise", "nlm", "--deblock", "weak", "--dering", "cdef", "--scan", "detect"])          # the stages go together
    assert a.denoise == "ata" and a.spatial_denoise == "nlm" and a.deblock == "weak" and a.dering == "cdef"
    for extra, words in ((["--dering-strength", "4,2"], "go with --dering cdef"),
                         (["--dering-damping", "5"], "go with --dering cdef"),
                         (["--dering", "none", "--dering-chroma-strength", "1,1"], "go with --dering cdef"),
                         (["--dering", "cdef", "--dering-damping", "7"], "--dering-damping = 7: an int in 3 .. 6"),
                         (["--dering", "cdef", "--dering-damping", "x"], "invalid int value"),
                         (["--dering", "cdef", "--dering-strength", "4"], "--dering-strength: P,S, got '4'"),
                         (["--dering", "cdef", "--dering-strength", "a,b"], "--dering-strength: P,S with integers"),
                         (["--dering", "cdef", "--dering-strength", "16,2"], "--dering-strength = (16, 2): two ints (p, s)"),
                         (["--dering", "cdef", "--dering-chroma-strength", "3,5"], "--dering-chroma-strength = (3, 5)"),
                         (["--dering", "strong"], "invalid choice")):
        with pytest.raises(SystemExit):
            parse_args(base + extra)
        assert words in capsys.readouterr().err, extra
    with pytest.raises(SystemExit):
        parse_args(png + ["--dering", "cdef", "--dering-chroma-strength", "2,2"])
    assert "goes with a Y4M input" in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------------------------------- the ABI
def test_header_binding_and_library_agree_at_abi_54():
    hdr = open(os.path.join(ROOT, "include", "savsr_hip.h")).read()
    assert int(re.search(r"#define\s+SAVSR_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 54
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    assert lib.savsr_abi_version() == _lib.ABI_VERSION
    for name in ("savsr_video_dering_u8", "savsr_video_dering_u16"):
        decl = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, plain, flags=re.S)
        assert decl, name
        params = [p.strip() for p in decl.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert len(params) == len(args), (name, params)
        for p, t in zip(params, args):          # pointers travel as void pointers, int64_t as c_int64, int as c_int
            want = _lib.C.c_void_p if "*" in p else _lib.C.c_int64 if p.startswith("int64_t") else _lib.C.c_int
            assert t is want, (name, p)
        assert hasattr(lib, name)
    names = [p.split()[-1].lstrip("*") for p in re.search(r"savsr_video_dering_u16\s*\((.*?)\);", plain, flags=re.S).group(1).split(",")]
    assert names == ["frames", "n_frames", "frame_bytes", "plane_offset", "rows", "cols", "step", "depth", "interlaced", "pri", "sec", "damping",
                     "out", "out_frame_bytes", "out_plane_offset", "stream"]
    build = open(os.path.join(ROOT, "savsr_amd", "csrc", "build.sh")).read()
    assert build.count("dering.hip") == 2
    assert callable(savsr_amd.dering_video) and savsr_amd.dering is dr
    # the entries refuse on the host, by name, before the device is touched
    assert lib.savsr_video_dering_u8(0, 1, 1, 0, 1, 1, 1, 0, 4, 2, 5, 0, 1, 0, None) == -1
    assert b"video_dering_u8: null pointer" in lib.savsr_last_error()
    buf = (_lib.C.c_uint8 * 256)()
    p = _lib.C.addressof(buf)
    for args, words in (((p, 1, 64, 0, 8, 8, 1, 0, 16, 2, 5, p + 128, 64, 0), b"video_dering_u8: pri a multiple of 1 << (depth - 8), 0 .. 15 << (depth - 8)"),
                        ((p, 1, 64, 0, 8, 8, 1, 0, 4, 5, 5, p + 128, 64, 0), b"video_dering_u8: sec a multiple of 1 << (depth - 8), 0 .. 4 << (depth - 8)"),
                        ((p, 1, 64, 0, 8, 8, 1, 0, 4, 2, 7, p + 128, 64, 0), b"video_dering_u8: damping 3 .. 6"),
                        ((p, 1, 64, 0, 8, 8, 1, 0, 4, 2, 5, p + 32, 64, 0), b"video_dering_u8: the source frames and the output overlap")):
        assert lib.savsr_video_dering_u8(*args, None) == -1 and words in lib.savsr_last_error(), args
    assert lib.savsr_video_dering_u16(p, 1, 128, 0, 8, 8, 1, 10, 0, 18, 8, 5, p + 128, 128, 0, None) == -1          # 18 is no multiple of 4
    assert b"video_dering_u16: pri a multiple" in lib.savsr_last_error()


# ---------------------------------------------------------------------------------------------------------------------- the host check
CXX = os.environ.get("CXX") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++"))


@pytest.mark.skipif(not CXX, reason="no clang++: the sanitizer build of the kernels' code needs one")
def test_the_kernels_code_passes_the_sanitizer_host_check():
    """tools/check_dering_host.py: csrc/dering.hip's entries and the three phases of its kernel as a stand-alone host program under
    ASan / UBSan, against the specification (the tool's docstring says what the host form covers and what only the GPU tests do)."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_dering_host.py"), "--cxx", CXX], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "cases equal the specification or are refused by name, no sanitizer report" in res.stdout
