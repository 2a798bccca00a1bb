"""tests/tail_cases.py on the CPU: its float64 references against torch's, the q builder against the 27-plane form, the two forms of the
source index against F.interpolate and against each other, every mutant outside the bound, and the bound not vacuous."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import tail_cases as TC

ALL_SHAPES = TC.separating_shapes() + [s for W in TC.EDGE_W for s in TC.edge_shapes(W)]


def _wt27(tw):
    """The projection of tests/test_gpu_kernels.py: row 3 (3 ky + kx) + o of the 27 x 64 matrix is tail.weight[o, :, ky, kx]."""
    m = torch.zeros(27, 64, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            for o in range(3):
                m[3 * (3 * ky + kx) + o] = tw[o, :, ky, kx]
    return m


def test_plane_reference_equals_conv2d(synth_sd):
    """Taps + bias of the 27-plane layout == F.conv2d in float64 of the un-projected feature map (to float64's own rounding)."""
    tw, tb = synth_sd["tail.weight"].double(), synth_sd["tail.bias"].double()
    for H, W in ((7, 9), (1, 5), (12, 33)):
        feat = torch.from_numpy(np.random.RandomState(H * W).standard_normal((64, H, W)))
        P = torch.einsum("pc,chw->phw", _wt27(tw), feat).numpy()
        A, S, n = TC.taps_planes(P)
        ref = F.conv2d(feat[None], tw, tb, padding=1)[0].numpy()
        assert np.abs(A + tb.numpy()[:, None, None] - ref).max() <= 1e-13 * (S.max() + 1)
        assert n.max() == min(H, 3) * 3 and n.min() == (2 if H > 1 else 1) * 2


@pytest.mark.parametrize("regime", TC.PLANE_REGIMES + TC.EXACT_REGIMES)
def test_q_builder_equals_the_27_plane_form(regime):
    for H, W in ((12, 33), (5, 64), (4, 97), (1, 31), (2, 32)) if regime != "onehot" else TC.ONEHOT_SHAPES:
        P, _ = TC.planes(regime, 3, H, W, 2)
        A27, S27, n27 = TC.taps_planes(P)
        Q, seam = TC.build_q(P)
        A, S, n = TC.taps_q(Q, seam)
        assert np.array_equal(A, A27), (regime, H, W)                   # exactly: every sum of multiples of 2^-30 is exact in float64
        assert n.max() <= 6 and bool((S <= S27).all())
        assert seam.size == TC.seam_floats(H, W)
        assert bool(np.isnan(seam[:, 0, 0]).all()) and bool(np.isnan(seam[:, -1, 1]).all())
        # the fp32 copies the kernel is given lose nothing of Q where three fp32 values of one magnitude are added, and never a seam
        assert np.array_equal(seam.astype(np.float32).astype(np.float64), seam, equal_nan=True)


def test_onehot_reference_is_the_plane_index_map():
    for nch in (1, 2, 3):
        H, W = TC.ONEHOT_SHAPES[0]
        P, bias = TC.planes("onehot", nch, H, W, 1)
        A, S, n = TC.taps_planes(P, nch)
        want = np.zeros_like(A)
        for p, (y, x) in enumerate(TC.onehot_positions(9 * nch, H, W, 1)):
            tap, o = divmod(p, nch)
            Y, X = y - tap // 3 + 1, x - tap % 3 + 1
            if 0 <= Y < H and 0 <= X < W:
                want[o, Y, X] = 1.0
        assert np.array_equal(A, want) and 0 < int(want.sum()) <= 9 * nch and float(A.max()) == 1.0
        assert not np.array_equal(TC.taps_planes(P, nch, transposed=True)[0], A)


def test_one_form_of_the_index_is_what_interpolate_computes():
    """The fused residual reference is within the arithmetic bound of F.interpolate on this CPU at every shape, or the plain one is (per
    axis: one of the four pairs).  Which one depends on how torch was compiled: recorded, not asserted."""
    ok = {fp: True for fp in TC.FORM_PAIRS}
    worst = {fp: 0.0 for fp in TC.FORM_PAIRS}
    for s in ALL_SHAPES:
        assert TC.lambda_is_inside(s.H, s.h) and TC.lambda_is_inside(s.W, s.w)
        for regime in ("uniform", "checker"):
            c = TC.center_frame(regime, 3, s.h, s.w, 1)
            got = F.interpolate(torch.from_numpy(c)[None], size=(s.H, s.W), mode="bilinear", align_corners=False)[0].numpy()
            for fp in TC.FORM_PAIRS:
                R, Rm = TC.residual(c, s, *fp)
                r = TC.ratio(got, R, TC.gamma(TC.K_INTERP + TC.K_FINAL) * Rm)
                worst[fp] = max(worst[fp], r)
                ok[fp] &= r <= 1.0
    print("F.interpolate on this CPU, worst |got - reference| / bound per (row form, column form):", {k: round(v, 2) for k, v in worst.items()},
          "-> matches", [fp for fp in TC.FORM_PAIRS if ok[fp]])
    assert any(ok.values()), worst


@pytest.mark.parametrize("k", range(3))
def test_the_two_forms_are_told_apart(k):
    """At each index-separating shape the forms differ at a coordinate, and their residuals differ by more than the bound at a pixel."""
    s = TC.separating_shapes()[k]
    dy, dx = TC.index_differences(s.H, s.h), TC.index_differences(s.W, s.w)
    print(s, "differing row / column indices:", dy, dx)
    assert (dy >= 1, dx >= 1) == ((True, False), (False, True), (True, True))[k]
    for regime in ("uniform", "checker"):
        c = TC.center_frame(regime, 3, s.h, s.w, 1)
        (Rf, Mf), (Rp, Mp) = TC.residual(c, s, "fused", "fused"), TC.residual(c, s, "plain", "plain")
        apart = np.abs(Rf - Rp) > 2 * TC.gamma(TC.K_INTERP + TC.K_FINAL) * np.maximum(Mf, Mp)          # no output can satisfy both
        print(s, regime, "pixels at which no output is within the bound of both forms:", int(apart.sum()), "max difference", float(np.abs(Rf - Rp).max()))
        assert int(apart.sum()) >= 1
        # and through the whole tail, on the planes the GPU file pins the index with
        P, bias = TC.planes("small", 3, s.H, s.W)
        taps = TC.taps_planes(P)
        ef, bf = TC.exact_and_bound(taps, bias, c, s, "fused", "fused")
        ep, bp = TC.exact_and_bound(taps, bias, c, s, "plain", "plain")
        assert int((np.abs(ef - ep) > bf + bp).sum()) >= 1


@pytest.mark.parametrize("name", list(TC.MUTANTS))
def test_every_mutant_leaves_the_bound(name):
    for layout in TC.MUTANTS[name][0]:
        for nch in ((1, 2, 3) if layout == "nch" else (3,)):
            if name == "bias_next" and nch == 1:
                continue                                                      # ((o + 1) % 1 is o)
            shape, P, bias, center = TC.mutant_inputs(layout, nch)
            cnt = []
            for fp in TC.FORM_PAIRS:
                good, bnd = TC.exact_and_bound(TC.layout_taps(layout, P, nch), bias, center, shape, *fp)
                bad, bnd2 = TC.mutant_reference(name, layout, P, bias, center, shape, *fp, nch=nch)
                assert np.array_equal(bnd, bnd2) and bool(np.isfinite(good).all())
                cnt.append(int(TC.outside(bad, good, bnd).sum()))
            print(f"{name:17s} {layout:3s} nch {nch}: outside the bound at {min(cnt)} of {good.size} outputs (the fewest of the four index forms)")
            assert min(cnt) >= 1


def test_the_bound_is_not_vacuous():
    """One tap of the exact result off by 2^-20 of the output's magnitude sum (16 u, above gamma(11)) puts that output outside."""
    for layout in ("p27", "q"):
        shape, P, bias, center = TC.mutant_inputs(layout)
        taps = TC.layout_taps(layout, P)
        exact, bnd = TC.exact_and_bound(taps, bias, center, shape, "fused", "fused")
        Rm = TC.residual(center, shape, "fused", "fused")[1]
        mag = taps[1] + np.abs(bias.astype(np.float64))[:, None, None] + Rm
        assert bool((bnd < 2.0 ** -20 * mag).all()) and bool((bnd > 0).all())
        assert bool(TC.outside(exact + 2.0 ** -20 * mag, exact, bnd).all())
        assert not bool(TC.outside(exact + 0.99 * bnd, exact, bnd).any())
    feat, wt, b = TC.conv_inputs("gauss", 5, 9)
    A, S, n = TC.taps_conv(feat, wt)
    ref = F.conv2d(torch.from_numpy(feat).double()[None], torch.from_numpy(wt).double(), padding=1)[0].numpy()
    assert np.abs(A - ref).max() <= 1e-13 * S.max() and int(n.max()) == 576


def test_conv_onehot_expected_is_the_weight():
    H, W = 24, 25
    feat, wt, b = TC.conv_inputs("onehot", H, W)
    A, S, n = TC.taps_conv(feat, wt)
    want = TC.onehot_conv_expected(wt, H, W)
    assert np.array_equal(A, want.astype(np.float64)) and int((want != 0).sum()) == 3 * 64 * 9


def test_mask_branch_references():
    x = np.random.RandomState(5).standard_normal((8, 10, 16)).astype(np.float32)
    t = torch.from_numpy(x).permute(2, 0, 1)[None]
    ref, b = TC.avgpool2_reference(x)
    assert np.abs(F.avg_pool2d(t, 2)[0].permute(1, 2, 0).numpy() - ref).max() <= b.max() and ref.shape == (4, 5, 16)
    ref, b = TC.upsample2x_reference(x)
    got = F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()
    assert ref.shape == (16, 20, 16) and bool((np.abs(got - ref) <= b).all())
