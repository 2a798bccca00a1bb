"""The CPU emulations of tests/range_cases.py satisfy, on their own, the conditions tests/test_gpu_conv_range.py relies on: in every
regime the three split products stay within the analytic worst case 3 * 2^-16 of each output's own S (S_wy in the Winograd-y form), fp32
accumulation of the same products stays within 2e-6 S of the float64 sum, outputs with S == 0 are exactly 0, the `addressed` regime
gives every (K chunk, tap) slot an owning channel, and a defect in one slot shows above the GPU tests' bound 2^-14 S in that channel.
Run with -s (or -rA) to read the worst ratios, quoted in units of 2^-17."""
import pytest
import torch

from tests import range_cases as R

# (cin, cout, ks, h, w)
SHAPES = [(128, 128, 3, 12, 33), (320, 64, 3, 9, 20), (16, 64, 3, 7, 34), (192, 64, 1, 7, 50)]
OWNED = [(128, 128, 3, 12, 33), (64, 64, 3, 12, 33), (16, 64, 3, 7, 34), (192, 64, 1, 7, 50)]      # cout >= nchunk * taps


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("cin,cout,ks,h,w", SHAPES)
def test_emulation_bounds(cin, cout, ks, h, w, regime):
    (_, x, wt), = R.regimes(cin, cout, ks, h, w, seed=cin * 7 + cout + h, only=(regime,))
    forms = [("direct", R.direct_emulation(x, wt, ks, acc32=True), "S")]
    exact = forms[0][1]["exact"]
    if ks == 3:
        forms.append(("winograd-y", R.wy_emulation(x, wt, acc32=True), "S_wy"))
    for form, e, skey in forms:
        s = e[skey]
        d_split, d_acc = (e["emul"] - exact).abs(), (e["acc32"] - e["emul"]).abs()
        line = f"{regime:9s} {cin}->{cout} ks{ks} {h}x{w} {form:10s}: split {R.ratio(d_split, s) / R.U17:6.3f} * 2^-17 {skey}, fp32 accumulation {R.ratio(d_acc, s):.2e} {skey}"
        if form == "winograd-y":
            line += f", against the direct S {R.ratio(d_split, forms[0][1]['S']) / R.U17:8.2f} * 2^-17, max S_wy/S {R.ratio(s, forms[0][1]['S']):.1f}"
        print(line)
        assert bool((d_split <= R.SPLIT_WORST * s).all())
        assert bool((d_acc <= R.T_ACC_CPU * s).all())
        assert bool((e["emul"][s == 0] == 0).all()) and bool((e["acc32"][s == 0] == 0).all())
    if regime == "sparse":
        assert bool((forms[0][1]["S"] == 0).any())                            # the exactness clause is not vacuous
        assert ks == 1 or bool((forms[1][1]["S_wy"] == 0).any())


@pytest.mark.parametrize("cin,cout,ks,h,w", OWNED)
def test_addressed_every_slot_has_an_owner(cin, cout, ks, h, w):
    """For each (chunk, tap) some channel has >= 99 % of its interior-pixel S from that slot -- and it is the channel slot_of names."""
    (_, x, wt), = R.regimes(cin, cout, ks, h, w, seed=cin * 7 + cout + h, only=("addressed",))      # (the draw R.case hands the GPU tests)
    taps, pad = ks * ks, ks // 2
    inner = (slice(None), slice(pad, h - pad), slice(pad, w - pad))
    s_all = R._conv(x.abs(), wt.abs(), pad)[inner].sum((1, 2))
    worst = 1.0
    for slot in range((cin // 16) * taps):
        chunk, tap = slot // taps, slot % taps
        wd = torch.zeros_like(wt)
        wd[:, 16 * chunk:16 * chunk + 16, tap // ks, tap % ks] = wt[:, 16 * chunk:16 * chunk + 16, tap // ks, tap % ks].abs()
        share = R._conv(x.abs(), wd, pad)[inner].sum((1, 2)) / s_all
        owners = [co for co in range(cout) if R.slot_of(co, cin, ks) == (chunk, tap)]
        assert owners and max(float(share[co]) for co in owners) >= 0.99, (slot, owners, share[owners])
        worst = min(worst, max(float(share[co]) for co in owners))
    print(f"addressed {cin}->{cout} ks{ks}: every one of {(cin // 16) * taps} slots owns >= {worst:.4f} of a channel's interior S")


def test_one_slot_defect_shows_above_the_gpu_bound():
    """x_lo w_hi missing in one (chunk, tap) slot of the direct form, the lo half of U missing in one (chunk, pos, kx) slot of the Winograd-y
    form: in `addressed`, an owning channel then has an output beyond 2^-14 S (S_wy) and beyond T_ACC S of the emulation; under Gaussian
    weights the same defect is diluted by 1 / K to a tenth of that or less."""
    cin, cout, h, w = 128, 128, 12, 33
    out = {}
    for regime in ("addressed", "gauss"):
        (_, x, wt), = R.regimes(cin, cout, 3, h, w, seed=2, only=(regime,))
        good, good_wy = R.direct_emulation(x, wt, 3), R.wy_emulation(x, wt)
        lo_d, hi_d, lo_w, hi_w = 1e30, 0.0, 1e30, 0.0
        for chunk in range(cin // 16):
            for tap in range(9):
                bad = R.direct_emulation(x, wt, 3, drop=(chunk, tap))
                err = (bad["emul"] - good["exact"]).abs()
                owners = [co for co in range(cout) if R.slot_of(co, cin, 3) == (chunk, tap)]
                r = max(R.ratio(err[co], good["S"][co]) for co in owners) if regime == "addressed" else R.ratio(err, good["S"])
                lo_d, hi_d = min(lo_d, r), max(hi_d, r)
                if regime == "addressed":
                    assert r > R.BOUND_EXACT, (chunk, tap, r)
                    assert max(R.ratio((bad["emul"] - good["emul"]).abs()[co], good["S"][co]) for co in owners) > R.T_ACC
            for pos in range(4):
                for kx in range(3):
                    bad = R.wy_emulation(x, wt, drop=(chunk, pos, kx))
                    err = (bad["emul"] - good["exact"]).abs()
                    owners = [co for co in range(cout) if R.slot_of(co, cin, 3)[0] == chunk and R.slot_of(co, cin, 3)[1] % 3 == kx
                              and R.slot_of(co, cin, 3)[1] // 3 in R.WY_TAPS_OF_POS[pos]]
                    r = max(R.ratio(err[co], good_wy["S_wy"][co]) for co in owners) if regime == "addressed" else R.ratio(err, good_wy["S_wy"])
                    lo_w, hi_w = min(lo_w, r), max(hi_w, r)
                    if regime == "addressed":
                        assert r > R.BOUND_EXACT, (chunk, pos, kx, r)
        out[regime] = (lo_d, hi_d, lo_w, hi_w)
        print(f"one-slot defect, {regime}: direct {lo_d / R.U17:.0f}-{hi_d / R.U17:.0f} * 2^-17 S, winograd-y {lo_w / R.U17:.0f}-{hi_w / R.U17:.0f} * 2^-17 S_wy")
    assert out["addressed"][0] > 10 * out["gauss"][1]          # 1 / K dilution: the regime shows the defect at full scale
