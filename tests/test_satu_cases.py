"""tests/satu_cases.py on the CPU: its float64 references against the oracle, what its regimes promise, its fp32 restatement of make_taps
against torch's grid_sample, and the sharpness of its bounds -- simulated defects in the emulations violate them in the outputs the defect's
slot dominates and nowhere else."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import savsr_oracle as O
from tests import satu_cases as SC
from tests.test_num_feat import p32_float64


def cpu_table(sd, h, w, sc) -> np.ndarray:
    """[H, W, 8] fp32 per-pixel table (r0 .. r3, off x y, soff x y) from the oracle's heads."""
    with torch.no_grad():
        off, soff, r = O.satu_heads(sd, "upsample", h, w, sc)
    return torch.cat([r[0], off[0], soff[0]], 0).permute(1, 2, 0).contiguous().numpy()


def _f32(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


@pytest.mark.parametrize("h,w,sc", [(6, 7, (4, 4)), (7, 6, (1.5, 4))])
def test_references_reproduce_the_oracle(h, w, sc):
    """synth / mlp / gauss: LR reference -> HR reference equals O.sta_upsample (plain form) and, contracted with Wt27, p32_float64 (p27
    form), to fp32 tolerance (the oracle runs in fp32; the references round the folded matrices and the record to fp32)."""
    sd = SC.weights("synth")
    x, st = SC.lr_data("gauss", 64, h, w)
    ax, tab = SC.unique_axes(h, w, sc), cpu_table(sd, h, w, sc)
    with torch.no_grad():
        ref = O.sta_upsample(sd, "upsample", x[None], sc, st[None])[0].double().numpy()
    got = SC.hr_reference(sd, 64, "plain", _f32(SC.lr_reference(sd, 64, "plain", x, st)["exact"]), tab, ax)["exact"]
    assert np.abs(got - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max())
    p32 = p32_float64(sd, 64, x[None], st[None], sc).numpy()
    got = SC.hr_reference(sd, 64, "p27", _f32(SC.lr_reference(sd, 64, "p27", x, st)["exact"]), tab, ax)["exact"]
    assert np.abs(got - p32).max() <= 2e-6 * max(1.0, np.abs(p32).max())
    assert np.abs(got[27:]).max() == 0.0


@pytest.mark.parametrize("form", ["plain", "p27", "q", "nf"])
def test_emulation_meets_the_bounds(form):
    """Without a defect the emulations sit well inside every bound, in every regime (the bounds are about the arithmetic, not the data)."""
    c = 32 if form == "nf" else 64
    h, w = 9, 33
    for ws, regimes in (("synth", SC.LR_REGIMES), ("wdecades", ("decades", "impulse")), ("negk", ("decades",)), ("addressed", ("impulse",))):
        sd = SC.weights(ws, c)
        for regime in regimes:
            r = SC.lr_reference(sd, c, form, *SC.lr_data(regime, c, h, w))
            assert bool((np.abs(r["emul"] - r["exact"]) <= 0.5 * r["bound"]).all()), (ws, regime)
    sd = SC.weights("synth", c)
    hh, ww, sc = 7, 6, (1.5, 4)
    ax = SC.unique_axes(hh, ww, sc)
    for heads in ("mlp", "half", "straddle", "wide"):
        tab = cpu_table(SC.with_heads(sd, heads, hh, ww), hh, ww, sc)
        for regime in ("gauss", "decades", "sparse"):
            rec = SC.hr_record(regime, 64 * SC.form_rows(form) // 32 + c // 2, hh, ww)
            r = SC.hr_reference(sd, c, form, rec, tab, ax, emul=True)
            assert bool((np.abs(r["emul"] - r["exact"]) <= 0.5 * r["bound"]).all()), (heads, regime)


def test_regimes_yield_what_they_promise():
    sd = SC.weights("synth")
    for h, w in SC.LR_SHAPES:
        r = SC.lr_reference(sd, 64, "p27", *SC.lr_data("hole", 64, h, w))
        for kind in range(3):                                  # the hole gives S_A = S_B = S_C = 0 somewhere, and nonzero S elsewhere
            s = r["S"][..., r["kind"] == kind]
            assert bool((s == 0).any()) and bool((s > 0).any()), (h, w, kind)
            assert bool((r["exact"][..., r["kind"] == kind][s == 0] == 0).all())
        assert len(set(SC.impulse_positions(64, h, w))) == min(64, h * w)
    # `addressed` x `impulse`: every slot (tap, channel group, k step) of kernel_conv dominates outputs of A (plain form) by >= 10^3
    sd, (x, st) = SC.weights("addressed"), SC.lr_data("impulse", 64, 9, 33)
    for tap, cg, ks in [(0, 0, 0), (7, 1, 2), (12, 0, 3), (24, 1, 1)]:
        r = SC.lr_reference(sd, 64, "plain", x, st, drop=("kconv", tap, cg, ks))
        dom = r["S_slot"] >= 1e3 * (r["S"] - r["S_slot"])
        assert int((dom & (r["S"] > 0)).sum()) >= 3, (tap, cg, ks)
    # head sets: positions in (-1, 0) and (size - 1, size) under `straddle`, on integers under `half`, every tap outside under `outside`
    for h, w, sc in SC.HR_SHAPES:
        ax = SC.unique_axes(h, w, sc)
        tab = cpu_table(SC.with_heads(sd, "straddle"), h, w, sc)
        lo_x = lo_y = hi_x = hi_y = False
        for which in range(2):
            ix, iy = SC.positions64(tab, ax, h, w, which)
            lo_x, hi_x = lo_x or bool(((ix > -1) & (ix < 0)).any()), hi_x or bool(((ix > w - 1) & (ix < w)).any())
            lo_y, hi_y = lo_y or bool(((iy > -1) & (iy < 0)).any()), hi_y or bool(((iy > h - 1) & (iy < h)).any())
        assert lo_x and hi_x and lo_y and hi_y, (h, w, sc)
        tab = cpu_table(SC.with_heads(sd, "outside", h, w), h, w, sc)
        for which in range(2):
            assert float(SC.taps32(tab, ax, h, w, which)["wgt"].max()) == 0.0
    on_integer = 0
    for h, w, sc in SC.HR_SHAPES:
        tab = cpu_table(SC.with_heads(sd, "half"), h, w, sc)
        for which in range(2):
            ix, iy = SC.positions64(tab, SC.unique_axes(h, w, sc), h, w, which)
            on_integer += int((np.abs(ix - np.round(ix)) < 1e-5).sum()) + int((np.abs(iy - np.round(iy)) < 1e-5).sum())
    assert on_integer > 0
    tab = cpu_table(SC.with_heads(sd, "r_sat"), 7, 6, (1.5, 4))
    assert bool((tab[..., [0, 2]] == 1.0).all()) and bool((tab[..., [1, 3]] < 1e-8).all())
    x, _ = SC.ramp(64, 9, 33)
    assert torch.equal(x, x.to(torch.bfloat16).float())


def test_make_taps32_agrees_with_grid_sample():
    """The fp32 restatement of make_taps against torch's grid_sample on one-hot images: the weight each pixel gets, within 2^-22, at
    positions inside, on integers, in the straddle bands and outside."""
    h, w = 5, 6
    g = np.random.RandomState(3)
    gx = np.concatenate([g.uniform(-1.6, 1.6, 200), np.linspace(-1, 1, w), [-1 - 1.0 / (w - 1), 1 + 1.0 / (w - 1), -1.2, 1.2, 3.0, -3.0]]).astype(np.float32)
    gy = np.concatenate([g.uniform(-1.6, 1.6, 200), np.tile(np.linspace(-1, 1, h), 2)[:w], [0.0, 0.0, -1.1, 1.1, -3.0, 3.0]]).astype(np.float32)
    t = SC.make_taps32(gx, gy, np.float32(0), np.float32(0), h, w)
    mine = np.zeros((len(gx), h, w))
    for k in range(4):
        np.add.at(mine, (np.arange(len(gx)), t["y0"] + (k >> 1) * t["dy"], t["x0"] + (k & 1) * t["dx"]), t["wgt"][k].astype(np.float64))
    onehot = torch.eye(h * w).view(1, h * w, h, w)
    grid = torch.from_numpy(np.stack([gx, gy], -1)).view(1, 1, -1, 2)
    ref = F.grid_sample(onehot, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, 0].t().reshape(-1, h, w).double().numpy()
    assert np.abs(mine - ref).max() <= 2.0 ** -22
    assert float(mine[-2:].max()) == 0.0 and float(mine.sum((1, 2)).max()) <= 1.0 + 2.0 ** -22


def _dominated(r, ratio=1e3):
    return (r["S_slot"] >= ratio * (r["S"] - r["S_slot"])) & (r["S"] > 0)


def _untouched(r):
    """Outputs whose S passes through the slot by <= 2^-7: a lost lo half (<= 2^-8 of a term) moves them by <= 2^-15 S, half of the tighter
    bound, on top of the clean emulation's own error (asserted <= half of the bound)."""
    return r["S_slot"] <= 2.0 ** -7 * r["S"]


def _sharp(r, tag, ratio=1e3):
    """The defect violates the bound in EVERY output its slot dominates (at least 3) and in no output the slot does not touch."""
    viol = np.abs(r["emul"] - r["exact"]) > r["bound"]
    dom = _dominated(r, ratio)
    print(tag, "dominated", int(dom.sum()), "violating", int(viol.sum()), "untouched", int(_untouched(r).sum()), "of", viol.size)
    assert int(dom.sum()) >= 3 and bool(viol[dom].all()) and not bool(viol[_untouched(r)].any())


@pytest.mark.parametrize("drop", [("kconv", 7, 1, 2), ("kconv", 24, 0, 0), ("wb", 1), ("wb", 3)])
def test_lr_defect_shows_where_its_slot_dominates_and_nowhere_else(drop):
    """`addressed` x `impulse`, plain form: the emulation without the lo half of one kernel_conv slot / one k step of Wb violates the bound
    against `exact` in every output that slot dominates and in none it does not touch."""
    sd, (x, st) = SC.weights("addressed"), SC.lr_data("impulse", 64, 9, 33)
    r = SC.lr_reference(sd, 64, "plain", x, st, drop=drop)
    _sharp(r, drop)
    clean = SC.lr_reference(sd, 64, "plain", x, st)
    assert not bool((np.abs(clean["emul"] - clean["exact"]) > 0.5 * clean["bound"]).any())


def _hr_addressed(h, w, sc, heads="mlp"):
    """`addressed` weights with a record whose (A, B) floats are 1e-4 of its C-stack: the expert product dominates every output."""
    sd = SC.weights("addressed")
    rec = SC.hr_record("gauss", 160, h, w).clone()
    rec[..., :128] *= 1e-4
    return sd, rec, cpu_table(SC.with_heads(sd, heads, h, w), h, w, sc), SC.unique_axes(h, w, sc)


@pytest.mark.parametrize("ks", [0, 1])
def test_hr_wbe_defect_shows_where_its_k_step_dominates(ks):
    h, w, sc = 7, 6, (1.5, 4)
    sd, rec, tab, ax = _hr_addressed(h, w, sc)
    r = SC.hr_reference(sd, 64, "plain", rec, tab, ax, defect=("wbe", ks))
    # (dominance >= 10^2 here: a row of Wb E has 16 entries of ~1e-4 in the other k step beside its one O(1) entry, the ratio cannot reach 10^3;
    # at a share of 0.99 the lost lo half, >= 2^-10 of the term, is still 15 x the bound)
    dom = _dominated(r, 1e2)
    rows = np.array([SC.expand_dominant(co)[0] // 2 == ks for co in range(64)])
    assert bool(dom[rows].any()) and not bool(dom[~rows].any())          # the rows whose dominant (n, j) lies in this k step
    _sharp(r, f"wbe k step {ks}", 1e2)


def test_hr_tap_defects_violate_the_bound():
    """A tap shifted by one column, and an out-of-image tap that keeps its weight: far outside the bound; the second only at pixels with a
    tap outside the image."""
    sd = SC.weights("synth")
    for h, w, sc in SC.HR_SHAPES[:3]:
        ax = SC.unique_axes(h, w, sc)
        tab = cpu_table(SC.with_heads(sd, "straddle"), h, w, sc)
        rec = SC.hr_record("gauss", 160, h, w)
        clean = SC.hr_reference(sd, 64, "plain", rec, tab, ax, emul=True)
        assert not bool((np.abs(clean["emul"] - clean["exact"]) > 0.5 * clean["bound"]).any())
        r = SC.hr_reference(sd, 64, "plain", rec, tab, ax, defect=("shift",))
        viol = np.abs(r["emul"] - r["exact"]) > r["bound"]
        assert float(viol.mean()) > 0.9
        r = SC.hr_reference(sd, 64, "plain", rec, tab, ax, defect=("nozero",))
        viol = (np.abs(r["emul"] - r["exact"]) > r["bound"]).any(0)
        band = np.zeros_like(viol)                     # pixels with a tap outside the image, in either gather
        for which in range(2):
            ix, iy = SC.positions64(tab, ax, h, w, which)
            band |= (ix < 0) | (ix > w - 1) | (iy < 0) | (iy > h - 1)
        assert int(viol.sum()) >= 3 and not bool((viol & ~band).any()) and int(viol.sum()) * 2 >= int(band.sum())


def test_group_helpers_name_the_lane_maps_groups():
    """packing.group_kconv / group_proj_tuned / group_wbe index the 512-element groups the lane maps produce (the device sharpness tests zero
    the lo half of a group found this way)."""
    from savsr_amd.packing import group_kconv, group_proj_tuned, group_wbe, lanes_a, lanes_acc, lanes_kconv, lanes_wbe
    for c in (32, 64):
        wk = np.arange(25 * c * c, dtype=np.float64).reshape(25 * c, c)
        img = lanes_kconv(wk, c).reshape(-1, 512)
        for tap, cg, ks in [(0, 0, 0), (7, c // 32 - 1, 2 % (c // 16)), (24, 0, c // 16 - 1)]:
            want = wk[25 * (32 * cg + np.arange(32)) + tap][:, 16 * ks:16 * ks + 16]
            assert sorted(img[group_kconv(tap, cg, ks, c)]) == sorted(want.reshape(-1))
    m = np.arange(64 * 64, dtype=np.float64).reshape(64, 64)
    cs = 10000.0 + np.arange(32 * 64, dtype=np.float64).reshape(32, 64)
    for ntiles in (1, 2):
        rows = 32 * ntiles
        ta, tb = m[:rows], 5000.0 + m[:rows]
        tiles = range(0, rows, 32)
        img = np.concatenate([a.reshape(-1) for a in [*(lanes_acc(ta, r) for r in tiles), *(lanes_a(tb, r) for r in tiles), lanes_a(cs)]]).reshape(-1, 512)
        for t in range(ntiles):
            for ks in range(4):
                assert sorted(img[group_proj_tuned(1, t, ks, ntiles)]) == sorted(tb[32 * t:32 * t + 32, 16 * ks:16 * ks + 16].reshape(-1))
                assert sorted(img[group_proj_tuned(0, t, ks, ntiles)]) == sorted(ta[32 * t:32 * t + 32, 32 * (ks // 2) + 16 * (ks % 2):][:, :16].reshape(-1))
        assert sorted(img[group_proj_tuned(2, 0, 3, ntiles)]) == sorted(cs[:, 48:64].reshape(-1))
        wbe = np.arange(4 * rows * 8, dtype=np.float64).reshape(4, rows, 8)
        img = np.concatenate([lanes_wbe(wbe, r).reshape(-1) for r in tiles]).reshape(-1, 512)
        for t in range(ntiles):
            for ks in range(2):
                assert sorted(img[group_wbe(t, ks)]) == sorted(wbe[2 * ks:2 * ks + 2, 32 * t:32 * t + 32].reshape(-1))
