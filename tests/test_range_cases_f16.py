"""The fp16 emulations of tests/range_cases.py satisfy, on their own, the conditions tests/test_gpu_conv_range_f16.py relies on: in every
finite regime the emulation stays within its derived per-output bound B (B_wy) of the exact value, fp32 accumulation of the same products
stays within 2e-6 S16 of the float64 sum, outputs with S16 == 0 are exactly 0; in `w_sub` / `x_sub` the same operands with subnormals flushed
miss B by more than 10x (so the GPU assertions tell a kernel that keeps subnormal operands from one that drops them); in `edge` the planted
values round as stated and an infinity reaches exactly the outputs whose receptive field holds it; and in `addressed` one slot of the weight
image rounded toward zero shows above the GPU tests' accumulation bound.  Run with -s (or -rA) to read the worst ratios."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import range_cases as R

# (cin, cout, ks, h, w): the direct shapes of tests/test_range_cases.py, the Winograd-y shapes of tests/test_gpu_conv_range.py
SHAPES = [(128, 128, 3, 12, 33), (320, 64, 3, 9, 20), (16, 64, 3, 7, 34), (192, 64, 1, 7, 50)]
WY = [(128, 128, 3, 12, 33), (128, 128, 3, 17, 34), (64, 64, 3, 36, 70)]
CASES = [(s, False) for s in SHAPES] + [(s, True) for s in WY]
IDS = [f"{'wy' if wy else 'direct'}-{s[0]}-{s[1]}-ks{s[2]}-{s[3]}x{s[4]}" for s, wy in CASES]


def _draw(shape, regime, **kw):
    cin, cout, ks, h, w = shape
    (_, x, wt), = R.regimes_f16(cin, cout, ks, h, w, seed=cin * 7 + cout + h, only=(regime,), **kw)      # (the draw R.case16 hands the GPU tests)
    return x, wt


def _emulate(shape, wy, x, wt, **kw):
    """(emulation, key of S16, key of B) of one form."""
    if wy:
        return R.f16_wy_emulation(x, wt, **kw), "S16_wy", "B_wy"
    return R.f16_direct_emulation(x, wt, shape[2], **kw), "S16", "B"


def test_regime_list_and_shared_draws():
    assert R.F16_REGIMES == ("gauss", "decades16", "matched", "mean50", "vsmooth", "altsign", "sparse", "heavy", "addressed", "w_sub", "x_sub", "edge")
    a = {n: (x, wt) for n, x, wt in R.regimes(16, 64, 3, 7, 34, seed=5)}
    b = {n: (x, wt) for n, x, wt in R.regimes_f16(16, 64, 3, 7, 34, seed=5)}
    assert tuple(b) == R.F16_REGIMES
    for n in R.REGIMES:
        if n != "decades":
            assert torch.equal(a[n][0], b[n][0]) and torch.equal(a[n][1], b[n][1]), n
    for n in R.F16_NEW:                                                    # a draw depends on (seed, name) only
        (_, x, wt), = R.regimes_f16(16, 64, 3, 7, 34, seed=5, only=(n,))
        assert torch.equal(x, b[n][0]) and torch.equal(wt, b[n][1]), n


@pytest.mark.parametrize("regime", R.F16_FINITE)
@pytest.mark.parametrize("shape,wy", CASES, ids=IDS)
def test_emulation_bounds(shape, wy, regime):
    x, wt = _draw(shape, regime)
    direct = R.f16_direct_emulation(x, wt, shape[2], acc32=not wy)
    e, skey, bkey = (R.f16_wy_emulation(x, wt, acc32=True), "S16_wy", "B_wy") if wy else (direct, "S16", "B")
    s16, bound = e[skey], e[bkey]
    d_round, d_acc = (e["emul"] - direct["exact"]).abs(), (e["acc32"] - e["emul"]).abs()
    sub_w, sub_x = float((wt.abs() < R.F16_MIN_NORMAL).double().mean()), float((x.abs() < R.F16_MIN_NORMAL).double().mean())
    print(f"{regime:9s} {shape[0]}->{shape[1]} ks{shape[2]} {shape[3]}x{shape[4]} {'winograd-y' if wy else 'direct':10s}: rounding {R.ratio(d_round, bound):.3f} of {bkey}, "
          f"fp32 accumulation {R.ratio(d_acc, s16):.2e} {skey}, fp16-subnormal or zero: {100 * sub_w:.1f} % of w, {100 * sub_x:.1f} % of x")
    assert bool(torch.isfinite(e["emul"]).all()) and bool(torch.isfinite(e["acc32"]).all())
    assert bool((d_round <= bound).all())
    assert bool((d_acc <= R.T_ACC_CPU * s16).all())
    assert bool((e["emul"][s16 == 0] == 0).all()) and bool((e["acc32"][s16 == 0] == 0).all())
    if regime == "sparse":
        assert bool((s16 == 0).any())                                      # the exactness clause is not vacuous
    if regime == "w_sub":
        assert sub_w == 1.0
    if regime == "x_sub":
        assert sub_x == 1.0


@pytest.mark.parametrize("shape,wy", CASES, ids=IDS)
def test_decades16_operands_stay_finite(shape, wy):
    """Every operand of `decades16`, and every Winograd-y U and V, is finite in fp16 (and well inside: the regime is about decades, not edges)."""
    from savsr_amd.packing import FP16_MAX, wy_transform_f64
    x, wt = _draw(shape, "decades16")
    mx, mw = float(x.abs().max()), float(wt.abs().max())
    line = f"decades16 {shape[0]}->{shape[1]} ks{shape[2]} {shape[3]}x{shape[4]}: max |x| {mx:.1f}, max |w| {mw:.1f}"
    assert mx <= FP16_MAX and mw <= FP16_MAX
    if shape[2] == 3:
        mu = float(np.abs(wy_transform_f64(wt)).max())
        xp = F.pad(x, (0, 0, 1, 3))
        mv = max(float((xp[:, i:i + x.shape[1]] + sg * xp[:, i + j:i + j + x.shape[1]]).abs().max()) for i, j, sg in ((0, 2, -1), (1, 1, 1), (1, 1, -1)))
        line += f", max |U| {mu:.1f}, max |V| {mv:.1f}"
        assert mu <= FP16_MAX and mv <= FP16_MAX
        e = R.f16_wy_emulation(x, wt)
        assert not bool(e["V_bad"].any())
    print(line)


@pytest.mark.parametrize("regime", ["w_sub", "x_sub"])
@pytest.mark.parametrize("shape,wy", CASES, ids=IDS)
def test_flushed_subnormals_miss_the_bound(shape, wy, regime):
    """The same operands with fp16 subnormals taken as zero: |flushed - exact| exceeds B (B_wy) by >= 10x somewhere, so bound 1 of the GPU
    tests (B + T_ACC S16) cannot be met by a kernel that flushes."""
    x, wt = _draw(shape, regime)
    exact = R._conv(x, wt, shape[2] // 2)
    e, skey, bkey = _emulate(shape, wy, x, wt, flush=True)
    clean, _, _ = _emulate(shape, wy, x, wt)
    r = R.ratio((e["emul"] - exact).abs(), clean[bkey])
    print(f"{regime} {shape[0]}->{shape[1]} ks{shape[2]} {shape[3]}x{shape[4]} {'winograd-y' if wy else 'direct'}: flushed operands miss {bkey} by {r:.1f}x")
    assert r >= 10.0
    assert R.ratio((e["emul"] - exact).abs(), clean[bkey] + R.T_ACC * clean[skey]) >= 10.0


def _fields(shape, wy, x, e):
    """[h, w] bool: the outputs whose receptive field holds an operand that is not finite in fp16 (direct: x; Winograd-y: V of the positions
    the output row combines, of the row pair's four input rows x 3 columns)."""
    _, _, ks, h, w = shape
    if not wy:
        bad = (x.abs() >= R.F16_INF_FROM).any(0).float()[None, None]
        return F.max_pool2d(bad, ks, 1, ks // 2)[0, 0] > 0
    vb = e["V_bad"].float()                                                # [4 pos][npair][w]
    wide = F.max_pool2d(vb[None], (1, 3), 1, (0, 1))[0] > 0
    r0, r1 = wide[0] | wide[1] | wide[2], wide[1] | wide[2] | wide[3]
    return torch.stack([r0, r1], 1).reshape(-1, w)[:h]


@pytest.mark.parametrize("shape,wy", CASES, ids=IDS)
def test_edge_on_the_emulation(shape, wy):
    cin, cout, ks, h, w = shape
    x, wt = _draw(shape, "edge")
    plants = R.edge_plants(h, w)
    assert len(plants) >= 4 or w < 17                                      # (every shape but the narrow ones carries the four single values)
    for what, ch, pts in plants:
        for r, c, v in pts:
            assert float(x[ch, r, c]) == v
    rnd = lambda v: float(R.f16_round(np.float32(v)))                      # noqa: E731
    assert rnd(65504.0) == 65504.0 and rnd(65519.0) == 65504.0 and rnd(65520.0) == np.inf and rnd(-70000.0) == -np.inf and rnd(40000.0) == 40000.0
    assert rnd(2.0 ** -25) == 0.0 and rnd(1.5 * 2.0 ** -25) == 2.0 ** -24 and rnd(2.0 ** -15) == 2.0 ** -15      # subnormals kept, RNE
    assert float(torch.tensor(65519.0).to(torch.float16)) == 65504.0 and float(torch.tensor(65520.0).to(torch.float16)) == np.inf
    assert bool((torch.from_numpy(R.f16_round(wt[:, :8].numpy())) != 0).all())      # no zero weight on a planted channel: an infinity poisons its whole field
    e, skey, bkey = _emulate(shape, wy, x, wt, acc32=True)
    cls = R.nonfinite_class(e["emul"])
    assert torch.equal(cls, R.nonfinite_class(e["acc32"]))                 # accumulation order and precision do not move a class
    field = _fields(shape, wy, x, e)
    assert torch.equal(cls != 0, field[None].expand_as(cls))                # every output of the field, and no other
    fin = cls == 0
    exact = R._conv(x, wt, ks // 2)
    assert bool(((e["emul"] - exact).abs()[fin] <= e[bkey][fin]).all())
    assert bool(((e["acc32"] - e["emul"]).abs()[fin] <= R.T_ACC_CPU * e[skey][fin]).all())
    names = [p[0] for p in plants]
    print(f"edge {cin}->{cout} ks{ks} {h}x{w} {'winograd-y' if wy else 'direct'}: plants {names}, non-finite outputs {int((cls != 0).sum())} "
          f"(+inf {int((cls == 1).sum())}, -inf {int((cls == 2).sum())}, NaN {int((cls == 3).sum())})")
    if "across pairs" in names:                                            # rows 7 and 8 add no non-finite output
        x2, _ = _draw(shape, "edge", skip_plants=("across pairs",))
        e2, _, _ = _emulate(shape, wy, x2, wt)
        assert torch.equal(R.nonfinite_class(e2["emul"]), cls)
    if wy:                                                                 # the Winograd-y form's non-finite set strictly contains the direct form's
        dcls = R.nonfinite_class(R.f16_direct_emulation(x, wt, ks)["emul"])
        assert bool(((dcls != 0) <= (cls != 0)).all()) and int((cls != 0).sum()) > int((dcls != 0).sum())
        # each of the three is finite in the direct form and not in this one: V1 = d1 + d2 and V2 = d2 - d1 enter both rows of their pair, V0 =
        # d0 - d2 (rows 1 and 3) the first row of the pair at 2 only
        for what, row in (("pair ++", 5), ("pair +-", 3), ("d0 - d2", 2)):
            assert what in names
            c = dict((p[0], p[2]) for p in plants)[what][0][1]
            assert bool((dcls[:, row, c] == 0).all()) and bool((cls[:, row, c] != 0).all()), what


@pytest.mark.parametrize("wy", [False, True])
def test_one_slot_rounded_toward_zero_shows(wy):
    """Sharpness precondition: in `addressed` (the dominant weights are fp16-normal) one (chunk, tap) group of fp16(w) -- one (chunk, pos, kx)
    group of fp16(U) -- rounded toward zero puts every owning channel beyond T_ACC S16 of the clean emulation."""
    shape = (128, 128, 3, 12, 33)
    cin, cout = shape[:2]
    x, wt = _draw(shape, "addressed")
    good, skey, _ = _emulate(shape, wy, x, wt)
    lo = 1e30
    for slot in ([(5, t) for t in range(9)] if not wy else [(5, p, k) for p in range(4) for k in range(3)]):
        bad, _, _ = _emulate(shape, wy, x, wt, drop=slot)
        if wy:
            owners = [co for co in range(cout) if R.slot_of(co, cin, 3)[0] == slot[0] and R.slot_of(co, cin, 3)[1] % 3 == slot[2]
                      and R.slot_of(co, cin, 3)[1] // 3 in R.WY_TAPS_OF_POS[slot[1]]]
        else:
            owners = [co for co in range(cout) if R.slot_of(co, cin, 3) == slot]
        assert owners
        for co in owners:
            r = R.ratio((bad["emul"] - good["emul"]).abs()[co], good[skey][co])
            lo = min(lo, r)
            assert r > R.T_ACC, (slot, co, r)
    print(f"one slot rounded toward zero, addressed, {'winograd-y' if wy else 'direct'}: every owner >= {lo:.2e} S16 = {lo / R.T_ACC:.0f} x T_ACC")
