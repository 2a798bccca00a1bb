"""The split-bf16 conv kernels (conv_mfma.hip direct 3x3 / 1x1, conv_wy.hip Winograd F(2,3) along y) across the dynamic-range regimes of
tests/range_cases.py, with PER-OUTPUT bounds relative to each output's own S = sum |x| |w| (S_wy for the Winograd form) instead of one
absolute number on Gaussian data.  The accumulators are observed directly: no bias, no activation, no residual.

Per output element:
  1. |got - exact| <= 2^-14 S          (split worst case 3 * 2^-16 = 0.75 of it, the rest is room for fp32 accumulation; derived)
  2. |got - emul|  <= T_ACC S          (emul: the same three split products summed in float64 -- only accumulation order and the fp32
                                        output transform may separate the kernel from it; T_ACC: see below)
  3. S == 0  =>  got == 0 exactly; nothing outside the output's channel slice is written.
The Winograd form's error relative to the DIRECT form's S is printed, not asserted: it grows with S_wy / S (the output transform's
cancellation; tests/test_range_cases.py prints the emulation's values: 0.1-0.5 * 2^-17 on Gaussian inputs, 6-11 on heavy tails, hundreds
to thousands where the dominant tap of an output falls on the zero padding or on zeros).

Measured on an MI355X (this file's own run, worst ratio over the shapes of each test):
  |got - exact|, direct, of S (* 2^-17):     gauss 0.08-0.35, decades 0.54-1.90, matched 0.08-0.45, mean50 0.06-0.25, vsmooth 0.08-0.43,
                                             altsign 0.07-0.26, sparse 0.38-2.11, heavy 1.25-2.14, addressed 1.13-1.35
  |got - exact|, Winograd-y, of S_wy:        gauss 0.12-0.19, decades 0.93-1.56, matched 0.12-0.19, mean50 0.14-0.19, vsmooth 0.21-0.32,
                                             altsign 0.10-0.30, sparse 0.62-0.86, heavy 1.16-1.83, addressed 0.83-0.94
  the same, of the DIRECT S (not asserted):  gauss 0.17-0.29, decades 2.0-4.5, matched 0.18-0.27, mean50 0.13-0.21, vsmooth 0.18-0.32,
                                             altsign 0.32-0.59, sparse 1.4-2.7, heavy 6.7-18.3, addressed 330-630
  |got - emul|, direct, of S (* 1e-6):       gauss 0.15, decades 1.09, matched 0.16, mean50 0.12, vsmooth 0.14, altsign 0.002, sparse 0.35,
                                             heavy 1.68, addressed 2.22 (320 -> 64; 0.47-1.41 at the other shapes); 16-row tiles, decades: 1.56
  |got - emul|, Winograd-y, of S_wy:         gauss 0.07, decades 0.41, matched 0.07, mean50 0.10, vsmooth 0.18, altsign 0.002, sparse 0.14,
                                             heavy 0.72, addressed 0.68
  T_ACC started at 2e-6; `addressed` 320 -> 64 in the direct form measured 2.22e-6 (below 2^-17 = 7.6e-6: accumulation, not a lost term -- 16
  dominant terms in the first K chunks, then 324 accumulator updates rounding at their scale; ATen's fp32 sum of the same products: 1.15e-6),
  so T_ACC = 1.5 x 2.22e-6 for every regime (tests/range_cases.py).
  pool rows: <= 2.7 * 2^-24 of the cell's sum |out| (bound 255 * 2^-24); whole network, 13 x 18 at (2.5, 3.5): 6.7e-6 (low-pass clip),
  4.9e-6 (constant 0.5), 9.4e-7 (all zero) max-abs against the fp32 oracle (bound 5e-5).
"""
import pytest
import torch

from savsr_amd.utils import synth
from tests import range_cases as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (cin, cout, ks, nsrc, h, w)
DIRECT = [(128, 128, 3, 2, 12, 33), (320, 64, 3, 5, 9, 20), (16, 64, 3, 1, 7, 34), (192, 64, 1, 3, 7, 50), (128, 64, 3, 1, 19, 11)]
# full tile with rows below the image; odd height + strip tile; several tiles
WY = [(128, 128, 12, 33), (128, 128, 17, 34), (64, 64, 36, 70)]


@pytest.fixture(scope="module")
def eng(synth_sd):
    from savsr_amd.engine import HipEngine
    from savsr_amd.archs.savsr_arch import SAVSR
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return HipEngine(synth_sd, SAVSR().cfg, DEV)


def cl(x):
    return x.permute(1, 2, 0).contiguous().to(DEV)


def pl(t):
    return t.detach().cpu().permute(2, 0, 1).contiguous()


def _image(wt, wy):
    from savsr_amd.packing import pack_conv_weight, pack_conv_weight_wy
    return (pack_conv_weight_wy(wt) if wy else pack_conv_weight(wt)).to(DEV)


class _Conv:
    """One conv's operands on the device and its descriptor: sources as channel slices of one tensor, the output as the slice [4, 4 + cout)
    of a NaN-filled wider tensor.  The descriptor holds raw pointers: the object keeps every tensor alive."""

    def __init__(self, eng, x, img, cout, ks, nsrc, algo, generic=False, pool=False):
        from savsr_amd import engine as E
        cin, h, w = x.shape
        sch = cin // nsrc
        self.cout, self.img = cout, img
        self.xall = cl(x)
        srcs = [eng.full(self.xall, sch, i * sch) for i in range(nsrc)]
        self.wide = torch.full((h, w, cout + 4), float("nan"), device=DEV)
        kw = {}
        if generic:      # a per-pixel mask of ones and a second residual of zeros: the generic epilogue instead of the straight-line one, same values
            self.mul, self.res2 = torch.ones(h, w, device=DEV), torch.zeros(h, w, cout, device=DEV)
            kw.update(mul_px=self.mul, res2=eng.full(self.res2), res2_scale=0.9)
        if pool:
            self.pool = torch.full((eng.pool_rows(h, w), cout + 4), float("nan"), device=DEV)
            kw["pool"] = (self.pool, 4, cout + 4)
        self.desc = eng.conv_desc("range", srcs, E.Src(self.wide, cout, cout + 4, 4), h, w, weights=(img, None, cout, cin, ks, algo), **kw)

    def result(self):
        assert bool(torch.isnan(self.wide[..., :4]).all())                # nothing written outside the channel slice
        return pl(self.wide[..., 4:]).double()


def _run(eng, x, img, cout, ks, nsrc, algo, **kw):
    c = _Conv(eng, x, img, cout, ks, nsrc, algo, **kw)
    eng.conv_launch([c.desc])
    torch.cuda.synchronize()
    return c.result()


def _check(tag, got, exact, emul, s, s_direct=None, t_acc=R.T_ACC, strict=True):
    """Assertions 1-3 on every output (strict), or only measured: returns the per-output pass masks of (1, 2) for the sharpness test."""
    e1, e2 = (got - exact).abs(), (got - emul).abs()
    line = f"{tag}: |got - exact| {R.ratio(e1, s) / R.U17:6.3f} * 2^-17 S, |got - emul| {R.ratio(e2, s):.2e} S"
    if s_direct is not None:
        line += f", against the direct S {R.ratio(e1, s_direct) / R.U17:8.2f} * 2^-17"
    print(line)
    ok1, ok2 = e1 <= R.BOUND_EXACT * s, e2 <= t_acc * s
    if strict:
        assert bool(torch.isfinite(got).all())
        assert bool(ok1.all()), (tag, "bound 1", R.ratio(e1, s) / R.BOUND_EXACT)
        assert bool(ok2.all()), (tag, "bound 2", R.ratio(e2, s) / t_acc)
        assert bool((got[s == 0] == 0).all()), (tag, "S == 0")
    return ok1, ok2


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("cin,cout,ks,nsrc,h,w", DIRECT)
def test_direct_per_output(eng, cin, cout, ks, nsrc, h, w, regime):
    """conv_mfma.hip, 8-row tiles: every regime at 128 -> 128 (two output blocks), 320 -> 64 from five sources, one K chunk (16 -> 64), 1x1
    and a narrow tall image."""
    from savsr_amd import _lib
    c = R.case(cin, cout, ks, h, w, regime)
    got = _run(eng, c["x"], _image(c["wt"], False), cout, ks, nsrc, _lib.CONV_DIRECT)
    _check(f"direct {regime:9s} {cin}->{cout} ks{ks} {h}x{w}", got, c["exact"], c["emul"], c["S"])
    if regime == "sparse":
        assert bool((c["S"] == 0).any())


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("cin,cout,h,w", WY)
def test_winograd_y_per_output(eng, cin, cout, h, w, regime):
    """conv_wy.hip, algos WINOGRAD_Y and WINOGRAD_Y_THROUGHPUT (strip tiles for the last rows): bit-identical, bounds relative to S_wy."""
    from savsr_amd import _lib
    c = R.case(cin, cout, 3, h, w, regime, True)
    img = _image(c["wt"], True)
    got = _run(eng, c["x"], img, cout, 3, 1, _lib.CONV_WINOGRAD_Y)
    got_tp = _run(eng, c["x"], img, cout, 3, 1, _lib.CONV_WINOGRAD_Y_THROUGHPUT)
    assert torch.equal(got, got_tp)
    _check(f"winograd-y {regime:9s} {cin}->{cout} {h}x{w}", got, c["exact"], c["emul_wy"], c["S_wy"], s_direct=c["S"])
    if regime == "sparse":
        assert bool((c["S_wy"] == 0).any())


@pytest.mark.parametrize("wy", [False, True])
@pytest.mark.parametrize("cin,cout,h,w", [(128, 128, 12, 33), (64, 64, 12, 33)])
def test_addressed_both_epilogues(eng, cin, cout, h, w, wy):
    """`addressed` (every (K chunk, tap) slot owns a channel) through the straight-line epilogue and through the generic one (mask of ones,
    second residual of zeros): same bounds, same bits."""
    from savsr_amd import _lib
    c = R.case(cin, cout, 3, h, w, "addressed", True)
    img, algo = _image(c["wt"], wy), _lib.CONV_WINOGRAD_Y if wy else _lib.CONV_DIRECT
    emul, s = (c["emul_wy"], c["S_wy"]) if wy else (c["emul"], c["S"])
    outs = []
    for generic in (False, True):
        got = _run(eng, c["x"], img, cout, 3, 1, algo, generic=generic)
        _check(f"addressed {'winograd-y' if wy else 'direct'} {cin}->{cout} generic={generic}", got, c["exact"], emul, s)
        outs.append(got)
    assert torch.equal(outs[0], outs[1])


def test_direct_16_row_tiles(eng):
    """`decades` at 64 -> 64, 100 x 320 in the 16-row tiling: algo DIRECT_THROUGHPUT takes it from 100 tiles of 16 rows, a lone conv of this
    shape has 70, so two convs share the launch (140; algo DIRECT would need 200 and stays on 8-row tiles).  Same bounds, bit-identical to
    DIRECT."""
    from savsr_amd import _lib
    cin, cout, h, w = 64, 64, 100, 320
    c = R.case(cin, cout, 3, h, w, "decades")
    img = _image(c["wt"], False)
    assert 2 * ((h + 15) // 16) * ((w + 31) // 32) >= 100 > ((h + 15) // 16) * ((w + 31) // 32)
    pair = [_Conv(eng, c["x"], img, cout, 3, 1, _lib.CONV_DIRECT_THROUGHPUT) for _ in range(2)]
    eng.conv_launch([p.desc for p in pair])
    ref8 = _run(eng, c["x"], img, cout, 3, 1, _lib.CONV_DIRECT)
    torch.cuda.synchronize()
    for k, p in enumerate(pair):
        got = p.result()
        assert torch.equal(got, ref8), k
    _check("direct 16-row decades 64->64 100x320", got, c["exact"], c["emul"], c["S"])


@pytest.mark.parametrize("wy", [False, True])
def test_one_launch_four_regimes(eng, wy):
    """One savsr_conv2d_batch of four 128 -> 64 12 x 33 convs, each in its own regime: each keeps its bounds and equals the same conv
    launched alone, bit for bit."""
    from savsr_amd import _lib
    cin, cout, h, w = 128, 64, 12, 33
    algo = _lib.CONV_WINOGRAD_Y if wy else _lib.CONV_DIRECT
    cases = [R.case(cin, cout, 3, h, w, r, True) for r in ("gauss", "decades", "mean50", "sparse")]
    imgs = [_image(c["wt"], wy) for c in cases]
    batch = [_Conv(eng, c["x"], img, cout, 3, 1, algo) for c, img in zip(cases, imgs)]
    alone = [_Conv(eng, c["x"], img, cout, 3, 1, algo) for c, img in zip(cases, imgs)]
    eng.conv_launch([b.desc for b in batch])
    for a in alone:
        eng.conv_launch([a.desc])
    torch.cuda.synchronize()
    for r, c, b, a in zip(("gauss", "decades", "mean50", "sparse"), cases, batch, alone):
        got = b.result()
        assert torch.equal(got, a.result()), r
        emul, s = (c["emul_wy"], c["S_wy"]) if wy else (c["emul"], c["S"])
        _check(f"batch of four, {'winograd-y' if wy else 'direct'} {r}", got, c["exact"], emul, s)


@pytest.mark.parametrize("wy", [False, True])
@pytest.mark.parametrize("regime", ["mean50", "decades"])
def test_fused_pool_partials(eng, regime, wy):
    """Every pool row (8-row band, 32-pixel segment) equals the float64 sum of the STORED outputs of its cell within 255 * 2^-24 sum |out| of
    that cell: the bound of any fp32 summation order of <= 256 terms.  19 x 40: a partial last band and a partial last segment."""
    from savsr_amd import _lib
    cin, cout, h, w = 128, 64, 19, 40
    c = R.case(cin, cout, 3, h, w, regime, True)
    cv = _Conv(eng, c["x"], _image(c["wt"], wy), cout, 3, 1, _lib.CONV_WINOGRAD_Y if wy else _lib.CONV_DIRECT, pool=True)
    eng.conv_launch([cv.desc])
    torch.cuda.synchronize()
    out = cv.result()
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


def test_sharpness_lo_half_of_one_slot_zeroed(eng):
    """The checks see a fault in ONE slot of the weight image: `addressed` in the Winograd form with the image's lo half zeroed for one
    (chunk, position, kx) group, edited on the host and handed to the unmodified kernel.  Assertions 1 and 2 fail in every channel that slot
    dominates and hold in every other channel."""
    from savsr_amd import _lib
    from savsr_amd.packing import conv_wy_pack_index, pack_conv_weight_wy
    cin, cout, h, w = 128, 128, 12, 33
    chunk, pos, kx = 5, 1, 2
    c = R.case(cin, cout, 3, h, w, "addressed", True)
    idx = conv_wy_pack_index(cout, cin)[0].reshape(4, cout, cin, 3)[pos, :, 16 * chunk:16 * chunk + 16, kx].reshape(-1)
    img = pack_conv_weight_wy(c["wt"]).view(-1, 2, 512).clone()                       # [group][hi, lo][512]
    assert bool((img[idx // 512, 1, idx % 512] != 0).any())
    img[idx // 512, 1, idx % 512] = 0
    got = _run(eng, c["x"], img.reshape(-1).to(DEV), cout, 3, 1, _lib.CONV_WINOGRAD_Y)
    ok1, ok2 = _check(f"sharpness: lo half zero at chunk {chunk} pos {pos} kx {kx}", got, c["exact"], c["emul_wy"], c["S_wy"], strict=False)
    hit = torch.tensor([R.slot_of(co, cin, 3)[0] == chunk and R.slot_of(co, cin, 3)[1] % 3 == kx
                        and R.slot_of(co, cin, 3)[1] // 3 in R.WY_TAPS_OF_POS[pos] for co in range(cout)])
    assert int(hit.sum()) >= 3
    assert not bool(ok1[hit].all(2).all(1).any()) and not bool(ok2[hit].all(2).all(1).any())      # seen in every channel of the slot ...
    # ... and nowhere else: bound 1 holds at every other output, bound 2 at every other output whose own dominant tap lies inside the image (in
    # the first and last column a channel whose tap reads the zero padding has no dominant slot left: S_wy is the sum of its 1e-4 weights,
    # and the 16 faulty ones among them show at 1 / 100 dilution instead of 1 / 10^5 -- above T_ACC, below bound 1)
    assert bool(ok1[~hit].all()) and bool(ok2[~hit][:, :, 1:w - 1].all())
    bad = R.wy_emulation(c["x"], c["wt"], drop=(chunk, pos, kx))["emul"]               # the emulation of the SAME defect explains the output
    assert bool(((got - bad).abs() <= R.T_ACC * c["S_wy"]).all())


def _clips(h, w):
    pic = synth.synth_gt(3, h, w + 6, seed=3)                                          # a low-pass picture drifting one pixel per frame
    return dict(lowpass=torch.stack([pic[:, :, t:t + w] for t in range(7)])[None].contiguous(),
                const=torch.full((1, 7, 3, h, w), 0.5), zero=torch.zeros(1, 7, 3, h, w))


@pytest.fixture(scope="module")
def net(synth_sd):
    import savsr_amd
    n = savsr_amd.build_network(dict(type="SAVSR")).eval()
    n.load_state_dict(synth_sd, strict=True)
    return n.to(DEV)


@pytest.mark.parametrize("clip", ["lowpass", "const", "zero"])
def test_network_on_non_noise_clips(net, synth_sd, clip):
    """The whole network where the activations are not noise: a smooth drifting picture, a constant clip, an all-zero clip, against the fp32
    oracle within the suite's end-to-end bound; finite; the eager launch sequence, the captured graphs' first run and a replay: same bits."""
    from oracle import savsr_oracle as O
    h, w, sc = 13, 18, (2.5, 3.5)
    lq = _clips(h, w)[clip]
    with torch.no_grad():
        ref = O.forward(synth_sd, lq, sc)
    dlq = lq.to(DEV)
    eager = torch.empty(3, round(h * sc[0]), round(w * sc[1]), device=DEV)
    net.engine().forward_one(dlq[0], sc, eager)
    net.set_scale(sc)
    a = net(dlq)
    b = net(dlq)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a).all())
    assert torch.equal(eager, a[0]) and torch.equal(a, b)
    err = float((a.cpu() - ref).abs().max())
    print(f"network on the {clip} clip: max-abs vs oracle {err:.3e} (output magnitude {float(ref.abs().max()):.2f})")
    assert err < 5e-5
