"""The noise estimator's specification (savsr_amd/noise.py) and everything around it that needs no GPU: the statistics against a slow
restatement, the hand-made cells, the decision on hand-made tables and on the synthetic pictures, the refusals, the ABI, the argument
checks of upscale_video / VideoUpscaler / the CLI, and the kernels' code under sanitizers as a host program."""
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
from savsr_amd import noise as NZ
from tests.noise_cases import (LARGE_SHAPE, SIGMAS, SMALL_SHAPE, case_seed, checkerboard, flat_beside_binned, picture, stats_frames, stats_plane,
                               true_sigma)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------- the statistics
def slow_stats(m, depth=8, interlaced=False):
    """`noise_stats_matrix` restated cell by cell with loops."""
    top = (1 << depth) - 1
    out = np.zeros((256, 2), np.int64)
    m = np.asarray(m)
    for plane in ((m[0::2], m[1::2]) if interlaced else (m,)):
        R, C = plane.shape
        v = [[min(int(s), top) for s in row] for row in plane]

        def L(y, x):
            def h(yy):
                return v[yy][x - 1] - 2 * v[yy][x] + v[yy][x + 1]
            return abs(h(y - 1) - 2 * h(y) + h(y + 1))
        for i in range(max(R - 2, 0) // 8):
            for j in range(max(C - 2, 0) // 8):
                cell = [[L(8 * i + 1 + a, 8 * j + 1 + b) for b in range(8)] for a in range(8)]
                rows = [sum(r) for r in cell]
                cols = [sum(cell[a][b] for a in range(8)) for b in range(8)]
                if 0 in rows or 0 in cols:
                    out[255, 0] += 1
                    continue
                S = sum(rows) >> (depth - 8)
                b = min(S >> 4, 254)
                out[b, 0] += 1
                out[b, 1] += S
    return out


@pytest.mark.parametrize("rows,cols,depth,interlaced", [(19, 27, 8, False), (26, 37, 8, True), (21, 20, 8, True), (23, 29, 10, False), (27, 18, 12, True),
                                                        (20, 21, 12, False)])
def test_stats_equal_the_slow_restatement(rows, cols, depth, interlaced):
    m = stats_plane(np.random.default_rng(case_seed(rows, cols, depth)), rows, cols, depth, above=True)
    got = NZ.noise_stats_matrix(m, depth, interlaced)
    assert np.array_equal(got, slow_stats(m, depth, interlaced))
    assert got[:255, 0].sum() > 0 and got.dtype == np.int64 and got.shape == (256, 2)
    if depth > 8:
        assert int(m.max()) > (1 << depth) - 1          # samples above the top are read as the top


def test_the_smallest_planes():
    rng = np.random.default_rng(case_seed(9, 9))
    for shape, cells in (((9, 9), 0), ((9, 40), 0), ((40, 9), 0), ((10, 10), 1), ((10, 18), 2), ((18, 10), 2), ((17, 17), 1), ((18, 18), 4)):
        assert NZ.noise_stats_matrix(rng.integers(0, 256, shape), 8)[:, 0].sum() == cells, shape
    m = rng.integers(0, 256, (20, 10))          # field-wise: two fields of 10 rows, one cell each; 19 rows: fields of 10 and 9 rows
    assert NZ.noise_stats_matrix(m, 8, True)[:, 0].sum() == 2 and NZ.noise_stats_matrix(m[:19], 8, True)[:, 0].sum() == 1
    assert NZ.noise_stats_matrix(m, 8, False)[:, 0].sum() == 2 and NZ.noise_stats_matrix(m[:19], 8, False)[:, 0].sum() == 2


def test_constant_planes_and_ramps_are_flat():
    y, x = np.mgrid[0:26, 0:34]
    for m in (np.full((26, 34), 77), 3 * x + 2 * y, 5 * x, x * y):
        t = NZ.noise_stats_matrix(m.astype(np.int64), 8)
        assert t[255, 0] == 12 and t[:255].sum() == 0 and t[255, 1] == 0


def test_one_zero_row_or_column_makes_a_cell_flat():
    rng = np.random.default_rng(case_seed(10, 10))
    m = rng.integers(0, 256, (10, 10))
    assert NZ.noise_stats_matrix(m, 8)[255, 0] == 0
    r = m.copy()
    r[3:6] = 40          # rows 3, 4, 5 constant: h is 0 there, so L of row 4 alone is 0
    t = NZ.noise_stats_matrix(r, 8)
    assert t[255, 0] == 1 and t[:255].sum() == 0
    c = m.copy()
    c[:, 5:8] = np.arange(10)[:, None]          # columns 5, 6, 7 equal: h of column 6 is 0 in every row
    t = NZ.noise_stats_matrix(c, 8)
    assert t[255, 0] == 1 and t[:255].sum() == 0
    t = NZ.noise_stats_matrix(flat_beside_binned(), 8)
    assert t[255, 0] == 1 and t[:255, 0].sum() == 1


def test_the_checkerboard_lands_in_the_last_bin_with_its_exact_sum():
    t = NZ.noise_stats_matrix(checkerboard(26, 34), 8)
    assert t[254, 0] == 12 and t[254, 1] == 12 * 64 * 2040 and t[:254].sum() == 0 and t[255].sum() == 0
    m12 = checkerboard(10, 10).astype(np.uint16) // 255 * 60000          # 12 bits: 0 / 4095 after the clamp, every L is 8 * 4095
    t = NZ.noise_stats_matrix(m12, 12)
    assert t[254, 0] == 1 and t[254, 1] == (64 * 8 * 4095) >> 4


def test_stats_keep_the_depths_fraction():
    m = picture(case_seed(10), 42, 50, 2.0, depth=10)
    t10 = NZ.noise_stats_matrix(m, 10)
    assert t10[:255, 1].sum() > 0 and not np.array_equal(t10, NZ.noise_stats_matrix(m >> 2, 8))


def test_stats_of_frames_by_class():
    rng = np.random.default_rng(case_seed(4, 4))
    v = stats_frames(rng, 2, 21, 27, step=3)
    t = NZ.noise_stats_frames(v)
    assert t.shape == (2, 2, 256, 2) and not t[:, 1].any()
    assert np.array_equal(t[1, 0], sum(NZ.noise_stats_matrix(v[1, :, :, ch]) for ch in range(3)))
    h, w = 36, 44
    y, cb, cr = (stats_plane(rng, *s, 12, True) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))
    f = np.concatenate([p.astype("<u2").reshape(-1).view(np.uint8) for p in (y, cb, cr)])[None]
    t = NZ.noise_stats_frames(f, "i420", (h, w), 12, True)
    assert np.array_equal(t[0, 0], NZ.noise_stats_matrix(y, 12, True))
    assert np.array_equal(t[0, 1], NZ.noise_stats_matrix(cb, 12, True) + NZ.noise_stats_matrix(cr, 12, True))
    assert not NZ.noise_stats_frames(np.zeros((1, 24 * 24), np.uint8), "y400", (24, 24))[:, 1].any()
    assert np.array_equal(NZ.noise_stats_frames(torch.from_numpy(v)), NZ.noise_stats_frames(v))


# ---------------------------------------------------------------------------------------------------------------------- the decision
def table_of(rows0, rows1=()):
    t = np.zeros((2, 256, 2), np.int64)
    for k, rows in enumerate((rows0, rows1)):
        for b, cnt, s in rows:
            t[k, b] = (cnt, s)
    return t


def test_the_rule_on_hand_made_tables():
    # 100 cells: k = 25; 10 from bin 3 at mean 50, 15 of the 30 of bin 5 at mean 2600 / 30
    v = NZ.verdict_from_stats(table_of([(3, 10, 500), (5, 30, 2600), (9, 60, 9000), (255, 7, 0)]))
    assert v.sigma == (Fraction(500) + Fraction(15 * 2600, 30)) / (245 * 25) and v.chroma_sigma is None and v.cells == (100, 0) and v.flat == (7, 0)
    # the quantile rounds up: 101 cells -> k = 26; quantile 1: the mean of all
    v = NZ.verdict_from_stats(table_of([(3, 10, 500), (5, 31, 2600), (9, 60, 9000)]))
    assert v.sigma == (Fraction(500) + Fraction(16 * 2600, 31)) / (245 * 26)
    v = NZ.verdict_from_stats(table_of([(3, 10, 500), (5, 30, 2600), (9, 60, 9000)]), quantile=1)
    assert v.sigma == Fraction(500 + 2600 + 9000, 245 * 100)
    # min_cells: 63 binned cells are too few, flat ones do not count; 64 are enough
    assert NZ.verdict_from_stats(table_of([(2, 63, 63 * 40), (255, 1000, 0)])).sigma is None
    assert NZ.verdict_from_stats(table_of([(2, 64, 64 * 40)])).sigma == Fraction(40, 245)
    assert NZ.verdict_from_stats(table_of([(2, 8, 8 * 40)]), min_cells=8).sigma == Fraction(40, 245)
    # the last bin takes part like any other
    assert NZ.verdict_from_stats(table_of([(254, 64, 64 * 130560)])).sigma == Fraction(130560, 245)
    # both classes on their own
    v = NZ.verdict_from_stats(table_of([(20, 64, 64 * 327)], [(10, 64, 64 * 163)]))
    assert v.sigma == Fraction(327, 245) and v.chroma_sigma == Fraction(163, 245) and v.cells == (64, 64)
    assert v.as_json()["sigma"]["fraction"] == [327, 245] and v.as_json()["cells"] == [64, 64] and len(v.as_json()["table"][0]) == 256


def verdict_at(sigma, chroma=None, floor=Fraction(1, 2)):
    return NZ.NoiseVerdict(sigma, chroma, (100, 100), (0, 0), np.zeros((2, 256, 2), np.int64), floor)


def test_both_maps():
    assert verdict_at(Fraction(2)).spatial_kwargs() == dict(spatial_strength=3.0)
    assert verdict_at(Fraction(4, 3)).denoise_kwargs() == dict(denoise_strength=(4, 9))
    assert verdict_at(Fraction(4, 3) + Fraction(1, 1000)).denoise_kwargs() == dict(denoise_strength=(5, 11))          # the ceiling
    assert verdict_at(Fraction(1)).spatial_kwargs() == dict(spatial_strength=1.5)
    assert verdict_at(Fraction(101, 100)).spatial_kwargs() == dict(spatial_strength=1.5)          # 24.24 + 0.5 -> 24 sixteenths
    assert verdict_at(Fraction(47, 48)).spatial_kwargs() == dict(spatial_strength=1.5)           # 23.5 + 0.5: half goes up
    assert verdict_at(Fraction(30)).spatial_kwargs() == dict(spatial_strength=32.0)
    assert verdict_at(Fraction(100)).denoise_kwargs() == dict(denoise_strength=(255, 255))
    assert verdict_at(Fraction(50)).denoise_kwargs() == dict(denoise_strength=(150, 255))
    # the floor: below it (and unknown) there is nothing to do; at it there is
    for v in (verdict_at(None), verdict_at(Fraction(49, 100)), verdict_at(None, Fraction(3))):
        assert v.spatial_kwargs() == {} and v.denoise_kwargs() == {}
    assert verdict_at(Fraction(1, 2)).spatial_kwargs() == dict(spatial_strength=0.75)
    assert verdict_at(Fraction(1, 2)).denoise_kwargs() == dict(denoise_strength=(2, 5))
    assert verdict_at(Fraction(1), floor=Fraction(2)).denoise_kwargs() == {}
    # chroma: the same maps; below the floor the spatial one reads the floor and the temporal one is the identity
    assert verdict_at(Fraction(2), Fraction(1)).spatial_kwargs() == dict(spatial_strength=3.0, spatial_chroma_strength=1.5)
    assert verdict_at(Fraction(2), Fraction(1, 10)).spatial_kwargs() == dict(spatial_strength=3.0, spatial_chroma_strength=0.75)
    assert verdict_at(Fraction(2), Fraction(1)).denoise_kwargs() == dict(denoise_strength=(6, 13), denoise_chroma_strength=(3, 7))
    assert verdict_at(Fraction(2), Fraction(1, 10)).denoise_kwargs() == dict(denoise_strength=(6, 13), denoise_chroma_strength=(0, 0))
    # the gains are parameters
    assert verdict_at(Fraction(2)).spatial_kwargs(gain=1) == dict(spatial_strength=2.0)
    assert verdict_at(Fraction(2)).denoise_kwargs(gain=Fraction(1, 2)) == dict(denoise_strength=(1, 3))
    # what the maps give passes the stages' own checks
    from savsr_amd.denoise import check_denoise_options
    from savsr_amd.nlmeans import check_spatial_options
    for s in (Fraction(1, 2), Fraction(7, 3), Fraction(300)):
        v = verdict_at(s, s / 7)
        check_denoise_options("ata", 4, **{k[len("denoise_"):]: x for k, x in v.denoise_kwargs().items()})
        check_spatial_options("nlm", 3, 7, **{k[len("spatial_"):]: x for k, x in v.spatial_kwargs().items()})


def sigma_of(m, depth=8, interlaced=False):
    t = np.zeros((2, 256, 2), np.int64)
    t[0] = NZ.noise_stats_matrix(m, depth, interlaced)
    return NZ.verdict_from_stats(t)


@pytest.mark.parametrize("sigma", SIGMAS)
def test_the_estimate_on_the_large_picture(sigma):
    for interlaced in (False, True):
        got = float(sigma_of(picture(case_seed(sigma, int(interlaced)), *LARGE_SHAPE, sigma), 8, interlaced).sigma)
        assert abs(got / true_sigma(sigma) - 1) <= 0.05, (sigma, interlaced, got)


@pytest.mark.parametrize("sigma", SIGMAS)
def test_the_estimate_on_the_small_picture(sigma):
    got = float(sigma_of(picture(case_seed(sigma, 2), *SMALL_SHAPE, sigma)).sigma)
    assert abs(got / true_sigma(sigma) - 1) <= 0.10, (sigma, got)


@pytest.mark.parametrize("sigma", SIGMAS)
def test_the_estimate_with_bars(sigma):
    v = sigma_of(picture(case_seed(sigma, 3), *LARGE_SHAPE, sigma, bars=True))
    assert abs(float(v.sigma) / true_sigma(sigma) - 1) <= 0.05, (sigma, float(v.sigma))
    assert v.flat[0] >= 2 * (LARGE_SHAPE[0] // 8 // 8 - 1) * ((LARGE_SHAPE[1] - 2) // 8)          # the bars' cells are flat, not read as quiet


def test_the_estimate_at_ten_bits_keeps_the_fraction():
    got = float(sigma_of(picture(case_seed(1, 4), *LARGE_SHAPE, 1.0, depth=10), 10).sigma)
    assert abs(got / float(np.sqrt(1.0 + 1.0 / (12 * 16))) - 1) <= 0.05, got


def test_no_noise_means_no_stage():
    v = sigma_of(picture(0, *LARGE_SHAPE, 0.0))
    assert v.sigma is not None and v.sigma < NZ.DEFAULT_FLOOR and v.spatial_kwargs() == {} and v.denoise_kwargs() == {}
    v = sigma_of(np.full(LARGE_SHAPE, 16, np.uint8))
    assert v.sigma is None and v.cells == (0, 0) and v.flat[0] == 35 * 43 and v.spatial_kwargs() == {}
    frames = np.stack([picture(case_seed(2, 5, t), 48, 64, 2.0) for t in range(3)])[..., None].repeat(3, -1)
    v = NZ.estimate_noise_frames(frames)
    assert v.cells[0] == 3 * 3 * 5 * 7 and abs(float(v.sigma) / true_sigma(2) - 1) <= 0.10


# ---------------------------------------------------------------------------------------------------------------------- the refusals
def test_every_refusal_by_name():
    t = np.zeros((2, 256, 2), np.int64)
    m = np.zeros((12, 12), np.uint8)
    bad_sum = t.copy()
    bad_sum[0, 255, 1] = 1
    for call, words in ((lambda: NZ.noise_stats_matrix(m.astype(np.float32)), r"the matrix must be \[R, C\] integers"),
                        (lambda: NZ.noise_stats_matrix(m[0]), r"the matrix must be \[R, C\] integers"),
                        (lambda: NZ.noise_stats_matrix(m[:0]), r"a matrix of 0 x 12"),
                        (lambda: NZ.noise_stats_matrix(m, 9), r"depth = 9: 8, 10 or 12"),
                        (lambda: NZ.noise_stats_frames(np.zeros((1, 3, 12, 12), np.float32)), r"float frames have no integer samples to measure noise in"),
                        (lambda: NZ.noise_stats_frames(np.zeros((1, 12, 12), np.uint8)), r"frames must be \[N, h, w, c\] uint8"),
                        (lambda: NZ.noise_stats_frames(np.zeros((1, 12, 12, 3), np.uint8), depth=10), r"depth = 10 goes with pixel_format"),
                        (lambda: NZ.noise_stats_frames(np.zeros((1, 100), np.uint8), "i420", (12, 12)), r"I420 frames of 12 x 12 are \[N, 216\] uint8"),
                        (lambda: NZ.verdict_from_stats(t[0]), r"table is \[2, 256, 2\] integers"),
                        (lambda: NZ.verdict_from_stats(t.astype(np.float64)), r"table is \[2, 256, 2\] integers"),
                        (lambda: NZ.verdict_from_stats(t - 1), r"counts and sums >= 0"),
                        (lambda: NZ.verdict_from_stats(bad_sum), r"no sum in row 255"),
                        (lambda: NZ.verdict_from_stats(t, quantile=0), r"quantile = 0: a number with 0 < q <= 1"),
                        (lambda: NZ.verdict_from_stats(t, quantile=1.5), r"quantile = 1\.5"),
                        (lambda: NZ.verdict_from_stats(t, quantile="a"), r"quantile = 'a'"),
                        (lambda: NZ.verdict_from_stats(t, quantile=True), r"quantile = True"),
                        (lambda: NZ.verdict_from_stats(t, min_cells=0), r"min_cells = 0: an int >= 1"),
                        (lambda: NZ.verdict_from_stats(t, min_cells=2.0), r"min_cells = 2\.0"),
                        (lambda: NZ.verdict_from_stats(t, floor=-1), r"floor = -1: a finite number >= 0"),
                        (lambda: NZ.verdict_from_stats(t, floor=float("nan")), r"floor = nan"),
                        (lambda: verdict_at(Fraction(2)).spatial_kwargs(gain=0), r"gain = 0: a finite number above 0"),
                        (lambda: verdict_at(Fraction(2)).denoise_kwargs(gain=float("inf")), r"gain = inf")):
        with pytest.raises(ValueError, match=words):
            call()
    doc = NZ.__doc__
    assert "this project's own" in doc and "synthetic pictures" in doc and "NOT validated on footage or on trained weights" in doc


def test_the_video_calls_refuse_before_the_gpu_is_touched():
    """upscale_video / VideoUpscaler on a network that is not on a GPU: every refusal is raised on the host, before the call would have
    asked for the device (a good call ends at that question)."""
    from savsr_amd import VideoUpscaler
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR(num_feat=32).eval()
    v = torch.zeros(8, 12, 16, 3, dtype=torch.uint8)
    for call in (lambda **kw: net.upscale_video(v, scale=2, out="uint8", **kw), lambda **kw: VideoUpscaler(net, 2, out="uint8", **kw)):
        for kw, words in ((dict(denoise_strength="auto"), r"denoise_strength = 'auto' goes with denoise=: without the stage there is nothing to set"),
                          (dict(spatial_strength="auto"), r"spatial_strength = 'auto' goes with spatial_denoise=: without the stage there is nothing to set"),
                          (dict(denoise="ata", denoise_strength="Auto"), r"denoise_strength = 'Auto'"),
                          (dict(spatial_denoise="nlm", spatial_strength="yes"), r"spatial_strength = 'yes'")):
            with pytest.raises(ValueError, match=words):
                call(**kw)
    for kw, words in ((dict(denoise="ata", denoise_strength="auto", denoise_radius=0), r"denoise_radius = 0"),
                      (dict(denoise="ata", denoise_strength="auto", denoise_chroma_strength=(3, 2)), r"denoise_chroma_strength = \(3, 2\)"),
                      (dict(spatial_denoise="nlm", spatial_strength="auto", spatial_search=9), r"spatial_search = 9"),
                      (dict(spatial_denoise="nlm", spatial_strength="auto", spatial_chroma_strength=0), r"spatial_chroma_strength = 0")):
        with pytest.raises(ValueError, match=words):
            net.upscale_video(v, scale=2, out="uint8", **kw)
    with pytest.raises(ValueError, match=r"denoise_strength = 'auto' in VideoUpscaler: the decision needs the whole video.*estimate_noise.*--denoise-strength auto"):
        VideoUpscaler(net, 2, out="uint8", denoise="ata", denoise_strength="auto")
    with pytest.raises(ValueError, match=r"spatial_strength = 'auto' in VideoUpscaler: the decision needs the whole video.*estimate_noise.*--spatial-strength auto"):
        VideoUpscaler(net, 2, out="uint8", spatial_denoise="nlm", spatial_strength="auto")
    for kw in (dict(denoise="ata", denoise_strength="auto"), dict(spatial_denoise="nlm", spatial_strength="auto")):
        with pytest.raises(ValueError, match="float frames"):
            net.upscale_video(torch.zeros(8, 3, 12, 16), scale=2, **kw)
        with pytest.raises(RuntimeError, match="AMD GPU only"):                      # a good call gets as far as the device
            net.upscale_video(v, scale=2, out="uint8", **kw)
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        net.upscale_video(v, scale=2, out="uint8", denoise="ata", denoise_strength="auto", spatial_denoise="nlm", spatial_strength="auto",
                          denoise_chroma_strength=(1, 2), spatial_chroma_strength=2.0, crop=(2, 2, 8, 12))
    # the explicit calls are what they were
    assert VideoUpscaler(net, 2, out="uint8", denoise="ata")._noise.strength == (4, 9)
    assert VideoUpscaler(net, 2, out="uint8", spatial_denoise="nlm")._grain == (3, 7, 3.0, 3.0)
    for call, words in ((lambda: savsr_amd.noise_stats(torch.zeros(2, 3, 4, 4)), r"float frames have no integer samples to measure noise in"),
                        (lambda: savsr_amd.estimate_noise(torch.zeros(2, 3, 4, 4)), r"float frames have no integer samples to measure noise in"),
                        (lambda: savsr_amd.estimate_noise(v, quantile=0), r"quantile = 0"),
                        (lambda: savsr_amd.estimate_noise(v, min_cells=0), r"min_cells = 0"),
                        (lambda: savsr_amd.estimate_noise(v, floor=-1), r"floor = -1"),
                        (lambda: savsr_amd.noise_stats(torch.zeros(2, 100, dtype=torch.uint8), "i420", (12, 16)), r"I420 frames of 12 x 16")):
        with pytest.raises(ValueError, match=words):
            call()


# ---------------------------------------------------------------------------------------------------------------------- the CLI
def test_cli_arguments(capsys):
    from savsr_amd.upscale import denoise_kwargs, parse_args, spatial_kwargs
    base = ["-i", "in.y4m", "-o", "out.y4m", "--scale", "2", "--checkpoint", "x.pth"]
    a = parse_args(base + ["--denoise", "ata", "--denoise-strength", "auto", "--noise-out", "n.json"])
    assert a.denoise_strength == "auto" and a.denoise_radius == 4 and a.noise_out == "n.json" and denoise_kwargs(a)["denoise_strength"] == "auto"
    a = parse_args(base + ["--spatial-denoise", "nlm", "--spatial-strength", "auto", "--spatial-chroma-strength", "2", "--crop", "auto", "--scan", "detect"])
    assert a.spatial_strength == "auto" and a.spatial_chroma_strength == 2.0 and a.spatial_patch == 3 and spatial_kwargs(a)["spatial_strength"] == "auto"
    png = ["-i", "in", "-o", "out", "--scale", "2", "--checkpoint", "x.pth"]
    a = parse_args(png + ["--denoise", "ata", "--denoise-strength", "auto", "--spatial-denoise", "nlm", "--spatial-strength", "auto"])
    assert (a.denoise_strength, a.spatial_strength) == ("auto", "auto")
    a = parse_args(base + ["--denoise", "ata", "--spatial-denoise", "nlm", "--spatial-strength", "4.5"])          # the explicit forms as they were
    assert a.denoise_strength == (4, 9) and a.spatial_strength == 4.5 and a.noise_out is None
    for extra, words in ((["--denoise-strength", "auto"], "go with --denoise ata"),
                         (["--spatial-strength", "auto"], "go with --spatial-denoise nlm"),
                         (["--noise-out", "n.json"], "--noise-out goes with --denoise-strength auto or --spatial-strength auto"),
                         (["--denoise", "ata", "--spatial-denoise", "nlm", "--noise-out", "n.json"], "--noise-out goes with"),
                         (["--denoise", "ata", "--denoise-strength", "Auto"], "--denoise-strength: A,B with integers"),
                         (["--spatial-denoise", "nlm", "--spatial-strength", "automatic"], "invalid float value"),
                         (["--spatial-denoise", "nlm", "--spatial-chroma-strength", "auto"], "invalid float value")):
        with pytest.raises(SystemExit):
            parse_args(base + extra)
        assert words in capsys.readouterr().err, extra
    for flags, name in ((["--denoise", "ata", "--denoise-strength", "auto"], "--denoise-strength"),
                        (["--spatial-denoise", "nlm", "--spatial-strength", "auto"], "--spatial-strength")):
        with pytest.raises(SystemExit):
            parse_args(["-i", "-", "-o", "out.y4m", "--scale", "2", "--checkpoint", "x.pth"] + flags)
        assert f"{name} auto needs a first pass over the input, which stdin does not allow" in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------------------------------- the ABI
def test_header_binding_and_library_agree_at_abi_55():
    hdr = open(os.path.join(ROOT, "include", "savsr_hip.h")).read()
    assert int(re.search(r"#define\s+SAVSR_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 55
    assert "(ABI 55) Noise statistics" in hdr
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    assert lib.savsr_abi_version() == _lib.ABI_VERSION
    for name in ("savsr_video_noise_stats_u8", "savsr_video_noise_stats_u16"):
        decl = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, plain, flags=re.S)
        assert decl, name
        params = [p.strip() for p in decl.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert len(params) == len(args), (name, params)
        for p, t in zip(params, args):          # pointers travel as void pointers, int64_t as c_int64, int as c_int
            want = _lib.C.c_void_p if "*" in p else _lib.C.c_int64 if p.startswith("int64_t") else _lib.C.c_int
            assert t is want, (name, p)
        assert hasattr(lib, name)
    names = [p.split()[-1].lstrip("*") for p in re.search(r"savsr_video_noise_stats_u16\s*\((.*?)\);", plain, flags=re.S).group(1).split(",")]
    assert names == ["frames", "n_frames", "frame_bytes", "plane_offset", "rows", "cols", "step", "depth", "interlaced", "out", "stream"]
    names = [p.split()[-1].lstrip("*") for p in re.search(r"savsr_video_noise_stats_u8\s*\((.*?)\);", plain, flags=re.S).group(1).split(",")]
    assert names == ["frames", "n_frames", "frame_bytes", "plane_offset", "rows", "cols", "step", "interlaced", "out", "stream"]
    build = open(os.path.join(ROOT, "savsr_amd", "csrc", "build.sh")).read()
    assert build.count(" noise.hip") == 2
    assert "savsr_video_noise_stats_u8" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert callable(savsr_amd.noise_stats) and callable(savsr_amd.estimate_noise) and savsr_amd.noise is NZ and savsr_amd.NoiseVerdict is NZ.NoiseVerdict
    # the entries refuse on the host, by name, before the device is touched
    assert lib.savsr_video_noise_stats_u8(0, 1, 1, 0, 1, 1, 1, 0, 0, None) == -1
    assert b"video_noise_stats_u8: null pointer" in lib.savsr_last_error()
    buf = (_lib.C.c_uint8 * 8192)()
    p = (_lib.C.addressof(buf) + 15) // 16 * 16
    q = p + 1024
    for args, words in (((p, 1, 64, 0, 8, 8, 1, 0, q + 4), b"video_noise_stats_u8: out must be 8-byte aligned"),
                        ((p, 1, 64, 0, 8, 8, 5, 0, q), b"video_noise_stats_u8: step 1 .. 4"),
                        ((p, 1, 64, 0, 8, 8, 0, 0, q), b"video_noise_stats_u8: step 1 .. 4"),
                        ((p, 0, 64, 0, 8, 8, 1, 0, q), b"video_noise_stats_u8: n_frames >= 1"),
                        ((p, 1, 64, 0, 0, 8, 1, 0, q), b"video_noise_stats_u8: rows >= 1"),
                        ((p, 1, 64, 0, 8, 0, 1, 0, q), b"video_noise_stats_u8: a row holds at least one sample"),
                        ((p, 1, 63, 0, 8, 8, 1, 0, q), b"video_noise_stats_u8: frame_bytes smaller"),
                        ((p, 1, 64, -1, 8, 8, 1, 0, q), b"video_noise_stats_u8: plane offsets >= 0"),
                        ((p, 1, 64, 0, 8, 8, 1, 2, q), b"video_noise_stats_u8: interlaced 0 or 1"),
                        ((p, 1, 64, 0, 8, 8, 1, 0, 0), b"video_noise_stats_u8: null pointer")):
        assert lib.savsr_video_noise_stats_u8(*args, None) == -1 and words in lib.savsr_last_error(), args
    for args, words in (((p, 1, 128, 0, 8, 8, 1, 9, 0, q), b"video_noise_stats_u16: depth 10 or 12 (8 bits: savsr_video_noise_stats_u8)"),
                        ((p + 1, 1, 128, 0, 8, 8, 1, 10, 0, q), b"video_noise_stats_u16: frames, the frame stride and the plane offset must be 2-byte aligned"),
                        ((p, 1, 129, 0, 8, 8, 1, 10, 0, q), b"2-byte aligned"),
                        ((p, 1, 128, 0, 8, 8, 1, 12, 3, q), b"video_noise_stats_u16: interlaced 0 or 1")):
        assert lib.savsr_video_noise_stats_u16(*args, None) == -1 and words in lib.savsr_last_error(), args


# ---------------------------------------------------------------------------------------------------------------------- the host check
CXX = os.environ.get("CXX") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++"))


@pytest.mark.skipif(not CXX, reason="no clang++: the sanitizer build of the kernels' code needs one")
def test_the_kernels_code_passes_the_sanitizer_host_check():
    """tools/check_noise_host.py: csrc/noise.hip's entries and device functions as a stand-alone host program under ASan / UBSan,
    against the specification (the tool's docstring says what the host form covers and what only the GPU tests do)."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_noise_host.py"), "--cxx", CXX], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "cases equal the specification or are refused by name, no sanitizer report" in res.stdout
