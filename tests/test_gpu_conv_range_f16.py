"""The fp16 forms of the conv kernels (savsr_conv2d_batch_f16: conv_mfma.hip direct 3x3 / 1x1, conv_wy.hip Winograd F(2,3) along y) and the
OSConv fp16 images across the regimes F16_REGIMES of tests/range_cases.py, with PER-OUTPUT bounds relative to each output's own
S16 = sum |fp16 x| |fp16 w| (S16_wy for the Winograd form), and at the ends of fp16's range: subnormal operands (`w_sub`, `x_sub`), values at
and beyond 65504 (`edge`).  The accumulators are observed directly: no bias, no activation, no residual.

Per output element, T = R.T_ACC (the project's bound for these accumulators in the split form, which feeds them three times the terms):
  1. |got - exact| <= B + T S16        (B: the derived bound of the fp16 roundings, range_cases.f16_err; no measurement enters)
  2. |got - emul|  <= T S16            (emul: the same fp16 operands, exact products, float64 sums)
  3. S16 == 0  =>  got == 0 exactly; every output finite; nothing outside the output's channel slice is written.
`w_sub` / `x_sub` under 1 and 2 are the subnormal-operand check: with subnormal fp16 operands taken as zero the emulation misses B by 24-144x
(tests/test_range_cases_f16.py).  In `edge`, the class (finite, +inf, -inf, NaN) of every output equals the emulation's, and 1-2 hold on
every finite output: an infinity reaches exactly the outputs whose receptive field holds it -- in the Winograd form the row pair's four
input rows x 3 columns, and from |x_a +- x_b| >= 65520 for rows one and two apart, where the direct form is still finite.

Measured on an MI355X (this file's own run, range over the shapes of each test):
  |got - exact|, direct, of B + T S16:       gauss 0.05-0.18, decades16 0.18-0.59, matched 0.05-0.18, mean50 0.03-0.12, vsmooth 0.04-0.16,
                                             altsign 0.02-0.11, sparse 0.23-0.74, heavy 0.41-0.72, addressed 0.42-0.53, w_sub 0.06-0.27,
                                             x_sub 0.06-0.31, edge (finite outputs) 0.57-0.71
  |got - exact|, Winograd-y, of B_wy + T S16_wy: gauss 0.06-0.09, decades16 0.21-0.37, matched 0.07-0.09, mean50 0.08-0.10, vsmooth 0.10-0.14,
                                             altsign 0.04-0.06, sparse 0.22-0.36, heavy 0.53-0.63, addressed 0.32-0.37, w_sub 0.09-0.13,
                                             x_sub 0.09-0.12, edge 0.52-0.67
  |got - emul|, direct, of S16 (* 1e-6):     gauss 0.10, decades16 0.34, matched 0.11, mean50 0.08, vsmooth 0.10, altsign 0.002, sparse 0.22,
                                             heavy 1.04, addressed 1.41 (320 -> 64), w_sub 0.11, x_sub 0.10, edge 1.65 (320 -> 64); 16-row
                                             tiles, decades16: 0.25
  |got - emul|, Winograd-y, of S16_wy:       gauss 0.05, decades16 0.24, matched 0.05, mean50 0.06, vsmooth 0.12, altsign 0.001, sparse 0.11,
                                             heavy 0.39, addressed 0.34, w_sub 0.05, x_sub 0.05, edge 0.70
  T = R.T_ACC = 3.33e-6 holds everywhere, unraised (the worst is half of it; ATen's fp32 sums of the same products: <= 1.18e-6).  The kernels
  KEEP subnormal fp16 operands: `w_sub` / `x_sub` sit at 5e-8 .. 1.1e-7 S16 of the subnormal-keeping emulation.
  edge: non-finite outputs direct 2304 / 1152 / 1152 / 128 / 0 (the 19 x 11 image is too narrow for an infinite plant), Winograd-y 5376 / 4992 /
  2112 against 2304 / 2304 / 1152 in the direct form of the same shapes; classes identical to the emulation, both algos, both epilogues.
  sharpness: the slot's owners at 5.2e-4 S16 (direct) and 3.9e-4 S16_wy (Winograd-y) of the clean emulation, 7.6e-7 / 3.2e-7 of the
  emulation of the same defect.  pool rows: <= 2.6 * 2^-24 of the cell's sum |out| (bound 255 * 2^-24).
  OSConv images: 0.500 fp16 steps at both ends, both forms (`high`: max |entry| 1581-1844 for 1.5 max |bank| = 60000).  With W'' summed in
  fp32, as the kernels did before this file, `high` measured 2.8 / 9.7 / 89 steps (c64 / c192 / c320) at the entries where sum_k ka W
  cancels to ~1e-5 of sum |ka W|: hidden by fp16's subnormal step at unit bank scale, and the reason the fp16 aggregation is in float64.
  whole network in fp16, 13 x 18 at (2.5, 3.5): lowpass 4.55e-4 / 9.18e-5 (0.93x / 0.99x the emulated max-abs / mean-abs), const 3.73e-4 /
  8.14e-5 (0.90x / 0.95x), zero 6.36e-5 / 1.74e-5 (0.78x / 1.01x).
"""
import os

import numpy as np
import pytest
import torch

from tests import range_cases as R
from tests.golden_cases import OSCONV_CASES, OSCONV_SCALES, rnd
from tests.test_gpu_conv_range import DEV, DIRECT, WY, _Conv, _clips, _run, cl

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = R.T_ACC


def _engine(sd):
    from savsr_amd.engine import HipEngine
    from savsr_amd.archs.savsr_arch import SAVSR
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    e = HipEngine(sd, SAVSR().cfg, DEV)
    e.precision = "fp16"              # every launch of this module: savsr_conv2d_batch_f16 / savsr_osconv_weights_batch_f16 on fp16 images
    return e


@pytest.fixture(scope="module")
def eng(synth_sd):
    return _engine(synth_sd)


def _image(wt, wy):
    from savsr_amd.packing import pack_conv_weight_f16, pack_conv_weight_wy_f16
    return (pack_conv_weight_wy_f16(wt) if wy else pack_conv_weight_f16(wt)).to(DEV)


def _keys(c, wy):
    return (c["emul_wy"], c["S16_wy"], c["B_wy"]) if wy else (c["emul"], c["S16"], c["B"])


def _check(tag, got, c, wy, emul=None, strict=True):
    """Assertions 1-3 on every output whose emulation is finite (strict), or only measured: returns the per-output pass mask of 2."""
    em, s16, b = _keys(c, wy)
    em = em if emul is None else emul
    fin = torch.isfinite(em)
    z = torch.zeros_like(em)
    e1, e2 = torch.where(fin, (got - c["exact"]).abs(), z), torch.where(fin, (got - em).abs(), z)
    b1, s = torch.where(fin, b + T * s16, z), torch.where(fin, s16, z)
    print(f"{tag}: |got - exact| {R.ratio(e1, b1):.3f} of B + T S16, |got - emul| {R.ratio(e2, s):.2e} S16")
    ok1, ok2 = e1 <= b1, e2 <= T * s
    if strict:
        assert torch.equal(R.nonfinite_class(got), R.nonfinite_class(em)), (tag, "classes")
        assert bool(ok1.all()), (tag, "bound 1", R.ratio(e1, b1))
        assert bool(ok2.all()), (tag, "bound 2", R.ratio(e2, s) / T)
        assert bool((got[fin & (s16 == 0)] == 0).all()), (tag, "S16 == 0")
    return ok2


@pytest.mark.parametrize("regime", R.F16_FINITE)
@pytest.mark.parametrize("cin,cout,ks,nsrc,h,w", DIRECT)
def test_direct_per_output(eng, cin, cout, ks, nsrc, h, w, regime):
    """conv_bf16x3_kernel<.., F16 = true>, 8-row tiles: every finite regime at 128 -> 128 (two output blocks), 320 -> 64 from five sources, one
    K chunk (16 -> 64), 1x1 and a narrow tall image."""
    from savsr_amd import _lib
    c = R.case16(cin, cout, ks, h, w, regime)
    got = _run(eng, c["x"], _image(c["wt"], False), cout, ks, nsrc, _lib.CONV_DIRECT)
    assert bool(torch.isfinite(got).all())
    _check(f"direct {regime:9s} {cin}->{cout} ks{ks} {h}x{w}", got, c, False)
    if regime == "sparse":
        assert bool((c["S16"] == 0).any())


@pytest.mark.parametrize("regime", R.F16_FINITE)
@pytest.mark.parametrize("cin,cout,h,w", WY)
def test_winograd_y_per_output(eng, cin, cout, h, w, regime):
    """conv_wy_kernel<FAST, true>, algos WINOGRAD_Y and WINOGRAD_Y_THROUGHPUT (strip tiles for the last rows): bit-identical, bounds relative
    to S16_wy."""
    from savsr_amd import _lib
    c = R.case16(cin, cout, 3, h, w, regime, True)
    img = _image(c["wt"], True)
    got = _run(eng, c["x"], img, cout, 3, 1, _lib.CONV_WINOGRAD_Y)
    got_tp = _run(eng, c["x"], img, cout, 3, 1, _lib.CONV_WINOGRAD_Y_THROUGHPUT)
    assert torch.equal(got, got_tp)
    assert bool(torch.isfinite(got).all())
    _check(f"winograd-y {regime:9s} {cin}->{cout} {h}x{w}", got, c, True)
    if regime == "sparse":
        assert bool((c["S16_wy"] == 0).any())


def _same(a, b):
    """Bit-identical where finite, the same class elsewhere (NaN != NaN)."""
    return torch.equal(R.nonfinite_class(a), R.nonfinite_class(b)) and torch.equal(torch.nan_to_num(a, 0.0, 0.0, 0.0), torch.nan_to_num(b, 0.0, 0.0, 0.0))


@pytest.mark.parametrize("cin,cout,ks,nsrc,h,w", DIRECT)
def test_edge_direct(eng, cin, cout, ks, nsrc, h, w):
    """`edge`, direct form: 65519 rounds to 65504 and stays finite, 65520 and -70000 are infinities that reach the outputs of their 3 x 3 (1 x 1)
    field and no other -- not the tile's other rows, not the other output block; +-40000 in neighbouring rows is finite."""
    from savsr_amd import _lib
    c = R.case16(cin, cout, ks, h, w, "edge")
    got = _run(eng, c["x"], _image(c["wt"], False), cout, ks, nsrc, _lib.CONV_DIRECT)
    print(f"edge direct {cin}->{cout} ks{ks} {h}x{w}: {int((~torch.isfinite(got)).sum())} non-finite outputs, emulation {int((~torch.isfinite(c['emul'])).sum())}")
    _check(f"edge direct {cin}->{cout} ks{ks} {h}x{w}", got, c, False)
    assert w < 17 or not bool(torch.isfinite(c["emul"]).all())


@pytest.mark.parametrize("cin,cout,h,w", WY)
def test_edge_winograd_y(eng, cin, cout, h, w):
    """`edge`, Winograd-y form, both algos: the emulation's classes, which hold strictly more non-finite outputs than the direct form's (V =
    d1 + d2, d2 - d1, d0 - d2 of +-40000 overflow); rows 7 and 8 (+40000 / +40000 across a pair boundary) stay finite."""
    from savsr_amd import _lib
    c = R.case16(cin, cout, 3, h, w, "edge", True)
    img = _image(c["wt"], True)
    got = _run(eng, c["x"], img, cout, 3, 1, _lib.CONV_WINOGRAD_Y)
    got_tp = _run(eng, c["x"], img, cout, 3, 1, _lib.CONV_WINOGRAD_Y_THROUGHPUT)
    assert _same(got, got_tp)
    nd, nw = int((~torch.isfinite(c["emul"])).sum()), int((~torch.isfinite(c["emul_wy"])).sum())
    print(f"edge winograd-y {cin}->{cout} {h}x{w}: {int((~torch.isfinite(got)).sum())} non-finite outputs, emulation {nw} (direct form {nd})")
    assert nw > nd
    _check(f"edge winograd-y {cin}->{cout} {h}x{w}", got, c, True)
    assert bool(torch.isfinite(got[:, 7:9, 30:33]).all())


@pytest.mark.parametrize("wy", [False, True])
def test_edge_generic_epilogue_and_batch_neighbour(eng, wy):
    """`edge` 128 -> 128 12 x 33 through the generic epilogue (mask of ones, second residual of zeros): the straight-line epilogue's bits and
    classes; and in one launch with a finite `gauss` conv: both equal their solo runs bit for bit."""
    from savsr_amd import _lib
    cin, cout, h, w = 128, 128, 12, 33
    algo = _lib.CONV_WINOGRAD_Y if wy else _lib.CONV_DIRECT
    ce, cg = R.case16(cin, cout, 3, h, w, "edge", True), R.case16(cin, cout, 3, h, w, "gauss", True)
    ie, ig = _image(ce["wt"], wy), _image(cg["wt"], wy)
    solo_e, solo_g = _run(eng, ce["x"], ie, cout, 3, 1, algo), _run(eng, cg["x"], ig, cout, 3, 1, algo)
    gen = _run(eng, ce["x"], ie, cout, 3, 1, algo, generic=True)
    _check(f"edge generic epilogue {'winograd-y' if wy else 'direct'}", gen, ce, wy)
    assert _same(gen, solo_e)
    pair = [_Conv(eng, ce["x"], ie, cout, 3, 1, algo), _Conv(eng, cg["x"], ig, cout, 3, 1, algo)]
    eng.conv_launch([p.desc for p in pair])
    torch.cuda.synchronize()
    assert _same(pair[0].result(), solo_e)
    assert torch.equal(pair[1].result(), solo_g) and bool(torch.isfinite(solo_g).all())
    _check(f"finite neighbour of edge {'winograd-y' if wy else 'direct'}", pair[1].result(), cg, wy)


def test_direct_16_row_tiles(eng):
    """`decades16` at 64 -> 64, 100 x 320 in the 16-row tiling (two convs share the launch, as tests/test_gpu_conv_range.py): same bounds,
    bit-identical to the 8-row tiling."""
    from savsr_amd import _lib
    cin, cout, h, w = 64, 64, 100, 320
    c = R.case16(cin, cout, 3, h, w, "decades16")
    img = _image(c["wt"], False)
    assert 2 * ((h + 15) // 16) * ((w + 31) // 32) >= 100 > ((h + 15) // 16) * ((w + 31) // 32)
    pair = [_Conv(eng, c["x"], img, cout, 3, 1, _lib.CONV_DIRECT_THROUGHPUT) for _ in range(2)]
    eng.conv_launch([p.desc for p in pair])
    ref8 = _run(eng, c["x"], img, cout, 3, 1, _lib.CONV_DIRECT)
    torch.cuda.synchronize()
    for k, p in enumerate(pair):
        got = p.result()
        assert torch.equal(got, ref8), k
    _check("direct 16-row decades16 64->64 100x320", got, c, False)


@pytest.mark.parametrize("wy", [False, True])
def test_one_launch_four_regimes(eng, wy):
    """One savsr_conv2d_batch_f16 of four 128 -> 64 12 x 33 convs, each in its own regime: each keeps its bounds and equals the same conv
    launched alone, bit for bit."""
    from savsr_amd import _lib
    cin, cout, h, w = 128, 64, 12, 33
    names = ("gauss", "decades16", "mean50", "w_sub")
    algo = _lib.CONV_WINOGRAD_Y if wy else _lib.CONV_DIRECT
    cases = [R.case16(cin, cout, 3, h, w, r, True) for r in names]
    imgs = [_image(c["wt"], wy) for c in cases]
    batch = [_Conv(eng, c["x"], img, cout, 3, 1, algo) for c, img in zip(cases, imgs)]
    alone = [_Conv(eng, c["x"], img, cout, 3, 1, algo) for c, img in zip(cases, imgs)]
    eng.conv_launch([b.desc for b in batch])
    for a in alone:
        eng.conv_launch([a.desc])
    torch.cuda.synchronize()
    for r, c, b, a in zip(names, cases, batch, alone):
        got = b.result()
        assert torch.equal(got, a.result()), r
        _check(f"batch of four, {'winograd-y' if wy else 'direct'} {r}", got, c, wy)


@pytest.mark.parametrize("wy", [False, True])
@pytest.mark.parametrize("regime", ["mean50", "decades16"])
def test_fused_pool_partials(eng, regime, wy):
    """Every pool row (8-row band, 32-pixel segment) equals the float64 sum of the STORED outputs of its cell within 255 * 2^-24 sum |out| of
    that cell: the bound of any fp32 summation order of <= 256 terms.  19 x 40: a partial last band and a partial last segment."""
    from savsr_amd import _lib
    cin, cout, h, w = 128, 64, 19, 40
    c = R.case16(cin, cout, 3, h, w, regime, True)
    cv = _Conv(eng, c["x"], _image(c["wt"], wy), cout, 3, 1, _lib.CONV_WINOGRAD_Y if wy else _lib.CONV_DIRECT, pool=True)
    eng.conv_launch([cv.desc])
    torch.cuda.synchronize()
    out = cv.result()
    _check(f"pool {regime} {'winograd-y' if wy else 'direct'}", out, c, wy)
    assert bool(torch.isnan(cv.pool[:, :4]).all())
    rows = cv.pool[:, 4:].double().cpu()
    ntx, worst = (w + 31) // 32, 0.0
    assert rows.shape[0] == ntx * ((h + 7) // 8)
    for band in range((h + 7) // 8):
        for seg in range(ntx):
            cell = out[:, 8 * band:8 * band + 8, 32 * seg:32 * seg + 32]
            err, mag = (rows[band * ntx + seg] - cell.sum((1, 2))).abs(), cell.abs().sum((1, 2))
            worst = max(worst, R.ratio(err, mag))
            assert bool((err <= 255 * 2.0 ** -24 * mag).all()), (band, seg)
    print(f"pool {regime} {'winograd-y' if wy else 'direct'}: worst row error {worst / 2.0 ** -24:.2f} * 2^-24 of its cell's sum |out|")


@pytest.mark.parametrize("wy", [False, True])
def test_sharpness_one_slot_rounded_toward_zero(eng, wy):
    """The checks see a fault in ONE slot of the fp16 weight image: `addressed` 128 -> 128 12 x 33 with the 16 channels of chunk 5 at tap 5
    (Winograd form: position 1, kx 2) rounded toward zero instead of to nearest, edited on the host and handed to the unmodified kernel.
    Assertion 2 fails in every channel that slot dominates and holds in every other channel; the emulation of the same defect explains the
    output."""
    from savsr_amd import _lib
    from savsr_amd.packing import conv_pack_index, conv_wy_pack_index, wy_transform_f64
    cin, cout, h, w = 128, 128, 12, 33
    chunk, pos, kx = 5, 1, 2
    tap = 3 * 1 + kx
    ch = slice(16 * chunk, 16 * chunk + 16)
    c = R.case16(cin, cout, 3, h, w, "addressed", True)
    if wy:
        idx = conv_wy_pack_index(cout, cin)[0].reshape(4, cout, cin, 3)[pos, :, ch, kx].reshape(-1)
        vals = R.f16_toward_zero(wy_transform_f64(c["wt"])[pos, :, ch, kx]).reshape(-1)
        bad = R.f16_wy_emulation(c["x"], c["wt"], drop=(chunk, pos, kx))["emul"]
        hit = torch.tensor([R.slot_of(co, cin, 3)[0] == chunk and R.slot_of(co, cin, 3)[1] % 3 == kx
                            and R.slot_of(co, cin, 3)[1] // 3 in R.WY_TAPS_OF_POS[pos] for co in range(cout)])
    else:
        idx = conv_pack_index(cout, cin, 3)[0].reshape(cout, cin, 9)[:, ch, tap].reshape(-1)
        vals = R.f16_toward_zero(c["wt"].double().numpy()[:, ch, tap // 3, tap % 3]).reshape(-1)
        bad = R.f16_direct_emulation(c["x"], c["wt"], 3, drop=(chunk, tap))["emul"]
        hit = torch.tensor([R.slot_of(co, cin, 3) == (chunk, tap) for co in range(cout)])
    img = _image(c["wt"], wy).cpu().numpy().view(np.float16).copy()
    assert int((img[idx] != vals).sum()) >= 16                                  # the defect moves weights (by one fp16 step each)
    img[idx] = vals
    form = "winograd-y" if wy else "direct"
    got = _run(eng, c["x"], torch.from_numpy(img.view(np.int16)).to(DEV), cout, 3, 1, _lib.CONV_WINOGRAD_Y if wy else _lib.CONV_DIRECT)
    ok2 = _check(f"sharpness {form}: chunk {chunk} {'pos %d kx %d' % (pos, kx) if wy else 'tap %d' % tap} toward zero", got, c, wy, strict=False)
    assert int(hit.sum()) >= (3 if wy else 1)
    assert not bool(ok2[hit].all(2).all(1).any())                                # seen in every channel of the slot ...
    # ... and nowhere else, at every output whose own dominant tap lies inside the image: at the border a channel whose tap reads the zero
    # padding has no dominant slot left, S16 is the sum of its 1e-4 weights (fp16-subnormal: 2^-24 steps on 2.5e-5), and the 16 of them the
    # defect moved show above T.  The Winograd form keeps the dominant weight in U1 / U2 at the first and last ROW, the direct form does not.
    inner = (slice(None), slice(None) if wy else slice(1, h - 1), slice(1, w - 1))
    assert bool(ok2[~hit][inner].all())
    s16 = _keys(c, wy)[1]
    assert bool(((got - bad).abs() <= T * s16).all())
    _check(f"sharpness {form}: against the emulation of the same defect", got, c, wy, emul=bad, strict=False)


def _att_weights(ent, bank, cin, cout):
    att = ent["att"].double().cpu()
    ca, fa, sa, ka = att[:cin], att[cin:cin + cout], att[cin + cout:cin + cout + 9], att[cin + cout + 9:]
    return fa.view(-1, 1, 1, 1) * ca.view(1, -1, 1, 1) * sa.view(1, 1, 3, 3) * (ka.view(-1, 1, 1, 1, 1) * bank).sum(0)


@pytest.fixture(scope="module")
def range_end_engines(synth_sd, eng):
    """Two engines on synth_sd with every OSConv bank rescaled: `high` -- 1.5 max |bank| = 60000 where the Winograd image exists (cout % 64
    == 0), else max |bank| = 60000: just inside _build_f16's check; `low` -- the bank's median magnitude 2^-18."""
    out = {}
    for end in ("high", "low"):
        sd = dict(synth_sd)
        for pfx, ent in eng.osc.items():
            bank = synth_sd[pfx + ".weight"]
            if end == "high":
                f = 60000.0 / (1.5 if ent["cout"] % 64 == 0 else 1.0) / float(bank.abs().max())
            else:
                f = 2.0 ** -18 / float(bank.abs().median())
            sd[pfx + ".weight"] = bank * f
        out[end] = (_engine(sd), sd)
    return out


@pytest.mark.parametrize("end", ["high", "low"])
@pytest.mark.parametrize("case,sc", list(zip(OSCONV_CASES, OSCONV_SCALES)), ids=[c[0] for c in OSCONV_CASES])
def test_osconv_f16_images_at_the_range_ends(range_end_engines, case, sc, end):
    """savsr_osconv_weights_batch_f16 where the bank sits at an end of fp16's range: every addressed entry of the direct and the Winograd-y
    image is finite and within 1 fp16 ulp of the float64 W'' (U) from the launch's own gates, unaddressed entries are zero.  `high` tests
    |U| <= 1.5 max |bank|, the claim _build_f16's range check rests on; `low`: more than half the entries are fp16-subnormal or zero."""
    from savsr_amd.packing import check_f16_range, conv_pack_index, conv_wy_pack_index, wy_transform_f64
    tag, pfx, cin = case
    e, sd = range_end_engines[end]
    h, w = 10, 12
    xall = cl(rnd((1, cin, h, w), 11 + cin, 0.7)[0])
    srcs = [e.full(xall, 64, i * 64) for i in range(cin // 64)]
    ent = e.osc[pfx]
    cout = ent["cout"]
    bank = sd[pfx + ".weight"].double()                                # [K, cout, cin, 3, 3]
    check_f16_range(pfx, bank.numpy() * (1.5 if cout % 64 == 0 else 1.0))          # (the engine accepts this checkpoint)
    for wy in (False, True) if cout % 64 == 0 else (False,):
        ent["wdyn"].fill_(0), ent["wdyn_wy"].fill_(0)
        e.osconv_weights(pfx, srcs, h, w, sc, wy=wy)
        torch.cuda.synchronize()
        wpp = _att_weights(ent, bank, cin, cout)
        if wy:
            idx, total = conv_wy_pack_index(cout, cin)
            ref = torch.from_numpy(wy_transform_f64(wpp)).reshape(-1)
            img = ent["wdyn_wy"]
        else:
            idx, total = conv_pack_index(cout, cin, 3)
            ref = wpp.reshape(-1)
            img = ent["wdyn"]
        got = img.view(torch.float16)[:total].cpu()
        vals = got[torch.from_numpy(idx)].double()
        assert bool(torch.isfinite(vals).all())
        ulp = torch.from_numpy(np.spacing(np.abs(ref.numpy()).astype(np.float16)).astype(np.float64))
        d = (vals - ref).abs() / ulp
        small = float((vals.abs() < R.F16_MIN_NORMAL).double().mean())
        print(f"{tag} {end} {sc} {'wy' if wy else 'direct'}: max ulp {float(d.max()):.3f}, max |entry| {float(vals.abs().max()):.4g} "
              f"(max |ref| {float(ref.abs().max()):.4g}, 1.5 max |bank| {1.5 * float(bank.abs().max()):.4g}), subnormal or zero {100 * small:.1f} %")
        assert float(d.max()) <= 1.0
        assert float(ref.abs().max()) <= (1.5 if wy else 1.0) * float(bank.abs().max())
        if end == "low":
            assert small > 0.5
        mask = torch.ones(total, dtype=torch.bool)
        mask[torch.from_numpy(idx)] = False
        assert not bool(got[mask].abs().max() > 0) if bool(mask.any()) else True


@pytest.fixture(scope="module")
def net16(synth_sd):
    import savsr_amd
    n = savsr_amd.build_network(dict(type="SAVSR")).eval()
    n.load_state_dict(synth_sd, strict=True)
    n.set_precision("fp16")
    return n.to(DEV)


@pytest.mark.parametrize("clip", ["lowpass", "const", "zero"])
def test_network_f16_on_non_noise_clips(net16, clip):
    """The whole network in fp16 mode where the activations are not noise (a smooth drifting picture, a constant clip, an all-zero clip),
    13 x 18 at (2.5, 3.5): finite; max-abs <= 3x and mean-abs <= 2x the CPU emulation's drift against the fp32 oracle (tools/
    gen_golden_precision.py --clips), with the fp32 suite's 5e-5 as the floor of either; eager = captured = replayed, bit for bit."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "precision_clips.npz"))
    h, w, sc = 13, 18, (2.5, 3.5)
    dlq = _clips(h, w)[clip].to(DEV)
    eager = torch.empty(3, round(h * sc[0]), round(w * sc[1]), device=DEV)
    net16.engine().forward_one(dlq[0], sc, eager)
    net16.set_scale(sc)
    a = net16(dlq)
    b = net16(dlq)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a).all())
    assert torch.equal(eager, a[0]) and torch.equal(a, b)
    d = np.abs(a[0].cpu().numpy().astype(np.float64) - g[f"{clip}/fp32"])
    emax, emean = (float(v) for v in g[f"{clip}/drift"])
    print(f"network fp16 on the {clip} clip: max-abs {d.max():.3e} ({d.max() / emax:.2f}x emulated {emax:.3e}), mean-abs {d.mean():.3e} ({d.mean() / emean:.2f}x {emean:.3e})")
    assert d.max() <= max(3 * emax, 5e-5) and d.mean() <= max(2 * emean, 5e-5)
