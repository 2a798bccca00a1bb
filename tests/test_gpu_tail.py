"""The kernels that write every frame -- savsr_tail_gather, savsr_tail_gather_nch, savsr_tail_gather_q, savsr_tail_residual -- and the OSAdapt
mask branch's savsr_avgpool2 / savsr_upsample2x through the C ABI against the float64 references of tests/tail_cases.py, per output, with
the bounds derived there (u = 2^-24 per rounding the kernel performs; nothing measured enters).  Every input plane is followed by NaN pitch
padding, the centre frame, the bias and the seams stand between NaNs, every seam entry the kernel must not read is a NaN, and every output
sits in a NaN-filled buffer whose guards are asserted afterwards.  A launch is judged against the residual reference under all four (row,
column) forms of the bilinear source index (`plain`: two roundings, `fused`: one); it passes where one of them holds the bound at every
output, and the index pin asserts that over the index-separating shapes exactly one pair is left, the same for every entry.

Measured on an MI355X (this file's own run, `pytest -s` prints the table at the end; a record, not a tolerance: every bound was derived
before the first run and none was adjusted).  Worst |got - exact| / bound under the index form that holds, per plane regime (max over
centre frames and shapes) -- `small` is the index pin's and the constant centre frame's planes of 2^-10:
  savsr_tail_gather      gauss 0.568, decades 0.627, altsign 0.637, small 0.470      (nch = 3 of savsr_tail_gather_nch: the same bits)
  savsr_tail_gather_nch  nch 1: 0.472 / 0.553 / 0.526 / 0.462; nch 2: 0.486 / 0.619 / 0.665 / 0.436
  savsr_tail_gather_q    gauss 0.707, decades 0.709, altsign 0.728, small 0.477
  savsr_tail_residual    gauss 0.006, decades 0.020 (576 sequential FMAs against gamma(578) S), small 0.157
  per centre frame (gather / q): uniform 0.627 / 0.728, checker 0.533 / 0.679, decades 0.632 / 0.726, constant 0.637 / 0.678
  savsr_avgpool2 gauss 0.831, decades 0.943; savsr_upsample2x gauss 0.763, decades 0.848; integers and onehot bit for bit on every entry.
Index pin: every entry (gather, nch 1 / 2 / 3, q, the conv kernel) holds its bound at the three separating shapes under (fused, fused)
alone: the kernels compute s = fma(scale, dst + 0.5, -0.5), one rounding, on both axes -- the form F.interpolate computes on the CPU.
Sharpness on the kernels' own outputs at 5 x 64: recip_scale 948, align_corners 942, i1_unclamped 204, lambda_unclamped 204, taps_transposed
960, pad_clamp 402, bias_next 960 of 960 outputs outside the bound; seam_at_x0 15, seam_right_edge 15, seam_swapped 30 (the seam columns).
What the first run found: where W % 4 == 0, savsr_tail_gather and savsr_tail_gather_q gave outputs up to 4 ulp apart (12 of 180 at 5 x 12)
depending on whether the pitch and the pointers allowed the 16-byte path, and savsr_tail_gather_nch at nch = 3 differed from
savsr_tail_gather in the same places; with a zero centre frame all agreed.  `(1.f - l) * a + l * b` had been contracted per instantiation:
one FMA per level on the 16-byte paths, packed products and an unfused sum on the one-pixel paths.  The kernels now spell the FMA form out
(lerp_fma, common.hpp) -- the 16-byte paths' instructions are unchanged -- and all of these are bitwise equal.
"""
import numpy as np
import pytest
import torch

from tests import tail_cases as TC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
F32 = np.float32
GUARD = 64                      # floats; 256 bytes, so a guarded pointer keeps the allocation's alignment
WORST = {}


@pytest.fixture(scope="module")
def lib():
    from savsr_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    so = _lib.load()
    _lib.check(so.savsr_prepare_device(), "savsr_prepare_device")
    yield so
    print("\nworst |got - exact| / bound per entry and regime (under the index form that holds):")
    for k in sorted(WORST):
        print(f"  {k[0]:12s} {k[1]:18s} {WORST[k]:.3f}")


def _note(entry, regime, r):
    WORST[(entry, regime)] = max(WORST.get((entry, regime), 0.0), r)


class Buf:
    """A float array on the device between two NaN guards, `off` floats behind the first (off = 1: a pointer that is not 16-byte aligned)."""

    def __init__(self, a=None, n=None, off=0):
        a = None if a is None else np.ascontiguousarray(a, dtype=F32).reshape(-1)
        self.n, self.lo = (n if a is None else a.size), GUARD + off
        self.t = torch.full((self.lo + self.n + GUARD,), NAN, device=DEV)
        if a is not None:
            self.t[self.lo:self.lo + self.n] = torch.from_numpy(a).to(DEV)
        self.ptr = self.t.data_ptr() + 4 * self.lo

    def guards_intact(self) -> bool:
        return bool(torch.isnan(self.t[:self.lo]).all()) and bool(torch.isnan(self.t[self.lo + self.n:]).all())

    def get(self) -> np.ndarray:
        torch.cuda.synchronize()
        assert self.guards_intact(), "written outside the output"
        return self.t[self.lo:self.lo + self.n].cpu().numpy()

    def untouched(self) -> bool:
        torch.cuda.synchronize()
        return bool(torch.isnan(self.t).all())


def _pitch(HW, mode):
    """Plane pitch in floats: at least 8 NaNs behind every plane; a multiple of 4 except in the `pitch` mode."""
    return (HW + 3) // 4 * 4 + 8 + (1 if mode == "pitch" else 0)


def _pitched(P, mode):
    """[n][H][W] -> (Buf of n planes of pitch _pitch, NaN between and behind them, pitch)."""
    n = P.shape[0]
    HW = P.shape[1] * P.shape[2]
    pitch = _pitch(HW, mode)
    a = np.full((n, pitch), np.nan, F32)
    a[:, :HW] = np.asarray(P, F32).reshape(n, HW)
    return Buf(a, off=1 if mode == "offset" else 0), pitch


def _modes(W):
    """vec: aligned pointers, pitch % 4 == 0 (the 16-byte path where W % 4 == 0).  The scalar fallbacks of a W % 4 == 0 launch: `pitch`
    (pitch % 4 != 0) and `offset` (planes and output one float off alignment)."""
    return ("vec", "pitch", "offset") if W % 4 == 0 else ("vec",)


def run_gather(lib, P, bias, center, s, mode="vec", nch=None):
    """savsr_tail_gather (nch = None) or savsr_tail_gather_nch -> [c][H][W]."""
    c = 3 if nch is None else nch
    pb, pitch = _pitched(P, mode)
    bb, cb = Buf(bias), Buf(center)
    out = Buf(n=c * s.H * s.W, off=1 if mode == "offset" else 0)
    if nch is None:
        rc = lib.savsr_tail_gather(pb.ptr, pitch, bb.ptr, cb.ptr, s.h, s.w, s.H, s.W, out.ptr, None)
    else:
        rc = lib.savsr_tail_gather_nch(pb.ptr, pitch, nch, bb.ptr, cb.ptr, s.h, s.w, s.H, s.W, out.ptr, None)
    assert rc == 0
    return out.get().reshape(c, s.H, s.W)


def q_inputs(P):
    """(Q, seam) in fp32 as the kernel is given them, from the float64 builder; the seam's never-read entries are NaN."""
    Q, seam = TC.build_q(P)
    return Q.astype(F32), seam.astype(F32)


def run_q(lib, Q, seam, bias, center, s, mode="vec"):
    qb, pitch = _pitched(Q, mode)
    sb, bb, cb = Buf(seam), Buf(bias), Buf(center)
    assert seam.size == TC.seam_floats(s.H, s.W)
    out = Buf(n=3 * s.H * s.W, off=1 if mode == "offset" else 0)
    assert lib.savsr_tail_gather_q(qb.ptr, pitch, sb.ptr, seam.size, bb.ptr, cb.ptr, s.h, s.w, s.H, s.W, out.ptr, None) == 0
    return out.get().reshape(3, s.H, s.W)


def run_conv(lib, feat, wt, bias, center, s, mode="vec"):
    assert mode in ("vec", "pitch")                                   # (the entry refuses a feature map that is not 16-byte aligned)
    fb, pitch = _pitched(feat, mode)
    wb, bb, cb = Buf(wt), Buf(bias), Buf(center)
    out = Buf(n=3 * s.H * s.W)
    assert lib.savsr_tail_residual(fb.ptr, pitch, wb.ptr, bb.ptr, cb.ptr, s.h, s.w, s.H, s.W, out.ptr, None) == 0
    return out.get().reshape(3, s.H, s.W)


def _same_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def _judged(entry, regime, got, taps, bias, center, s):
    """The set of index-form pairs under which `got` holds the bound everywhere; asserts it is not empty."""
    assert bool(np.isfinite(got).all()), (entry, regime, s)
    v = TC.judge(got, taps, bias, center, s)
    ok = TC.passing(v)
    assert ok, (entry, regime, s, v)
    _note(entry, regime, min(v.values()))
    return ok


def _cases(s, nch=3):
    for regime in TC.PLANE_REGIMES:
        P, bias = TC.planes(regime, nch, s.H, s.W)
        for cr in TC.CENTER_REGIMES:
            yield f"{regime}/{cr}", P, bias, TC.center_frame(cr, nch, s.h, s.w)


def _check_gather(lib, s):
    held = set(TC.FORM_PAIRS)
    for name, P, bias, center in _cases(s):
        taps = TC.taps_planes(P)
        got = run_gather(lib, P, bias, center, s)
        held &= _judged("gather", name, got, taps, bias, center, s)
        for mode in _modes(s.W)[1:]:
            assert _same_bits(run_gather(lib, P, bias, center, s, mode), got), (s, name, mode)      # the same summation order
    return held


def _check_nch(lib, s):
    held = set(TC.FORM_PAIRS)
    for nch in (1, 2, 3):
        for name, P, bias, center in _cases(s, nch):
            got = run_gather(lib, P, bias, center, s, nch=nch)
            held &= _judged(f"nch {nch}", name, got, TC.taps_planes(P, nch), bias, center, s)
            if nch == 3:
                assert _same_bits(got, run_gather(lib, P, bias, center, s)), (s, name)              # savsr_tail_gather's order
    return held


def _check_q(lib, s):
    held = set(TC.FORM_PAIRS)
    for name, P, bias, center in _cases(s):
        Q, seam = q_inputs(P)
        taps = TC.taps_q(Q, seam)
        got = run_q(lib, Q, seam, bias, center, s)
        held &= _judged("q", name, got, taps, bias, center, s)
        for mode in _modes(s.W)[1:]:
            assert _same_bits(run_q(lib, Q, seam, bias, center, s, mode), got), (s, name, mode)
    return held


@pytest.mark.parametrize("W", TC.EDGE_W)
def test_tail_gather_edges(lib, W):
    """savsr_tail_gather, plane regimes x centre frames, every edge height at edge width W; where W % 4 == 0 the 16-byte path and both
    scalar fallbacks, bit for bit the same."""
    for s in TC.edge_shapes(W):
        print(s, "holds under", sorted(_check_gather(lib, s)))


@pytest.mark.parametrize("W", TC.EDGE_W)
def test_tail_gather_nch_edges(lib, W):
    """savsr_tail_gather_nch for nch 1, 2, 3; at nch = 3 the bits of savsr_tail_gather on the same planes."""
    for s in TC.edge_shapes(W):
        print(s, "holds under", sorted(_check_nch(lib, s)))


@pytest.mark.parametrize("W", TC.EDGE_W)
def test_tail_gather_q_edges(lib, W):
    """savsr_tail_gather_q on synthetic Q and seams (tests/tail_cases.py, build_q) with non-zero centre frames; a NaN in every seam entry
    it must not read and behind seam_floats."""
    for s in TC.edge_shapes(W):
        print(s, "holds under", sorted(_check_q(lib, s)))


CONV_SHAPES = (TC.edge_shape(24, 68, (2.95, 3.75)), TC.edge_shape(24, 67, (1.5, 1.3)))     # two 16-byte-staged tiles and a partial one; W % 4 != 0


@pytest.mark.parametrize("k", range(2), ids=["W68", "W67"])
def test_tail_residual(lib, k):
    """The 64 -> 3 conv kernel: gauss and decades within the bound counted over its 576 FMAs; an impulse per channel returns the tail
    weights bit for bit; integers bit for bit.  W = 68 with a pitch % 4 == 0 stages two tiles with 16-byte loads (and once more with
    pitch % 4 != 0, the same bits); W = 67 stages every tile by scalars."""
    s = CONV_SHAPES[k]
    for regime in ("gauss", "decades"):
        feat, wt, bias = TC.conv_inputs(regime, s.H, s.W)
        center = TC.center_frame("uniform" if regime == "gauss" else "decades", 3, s.h, s.w)
        got = run_conv(lib, feat, wt, bias, center, s)
        print(s, regime, "holds under", sorted(_judged("conv", regime, got, TC.taps_conv(feat, wt), bias, center, s)))
        if s.W % 4 == 0:
            assert _same_bits(run_conv(lib, feat, wt, bias, center, s, "pitch"), got)
    zero = TC.center_frame("zero", 3, s.h, s.w)
    feat, wt, bias = TC.conv_inputs("onehot", s.H, s.W)
    for mode in ("vec", "pitch"):
        assert np.array_equal(run_conv(lib, feat, wt, bias, zero, s, mode), TC.onehot_conv_expected(wt, s.H, s.W)), mode
    feat, wt, bias = TC.conv_inputs("integers", s.H, s.W)
    A = TC.taps_conv(feat, wt)[0] + bias.astype(np.float64)[:, None, None]
    assert np.array_equal(run_conv(lib, feat, wt, bias, zero, s).astype(np.float64), A)


@pytest.mark.parametrize("H,W", TC.ONEHOT_SHAPES + ((5, 65),))
def test_exact_regimes(lib, H, W):
    """`integers` (integer planes and bias, centre 0) and `onehot` (one 1.0 per plane, 3 pixels apart: the plane-index map) bit for bit, on
    the three gather entries and every path of each."""
    s = TC.edge_shape(H, W, (2.95, 3.75))
    for regime in TC.EXACT_REGIMES:
        if regime == "onehot" and (H, W) not in TC.ONEHOT_SHAPES:
            continue
        for nch in (1, 2, 3):
            P, bias = TC.planes(regime, nch, H, W)
            zero = TC.center_frame("zero", nch, s.h, s.w)
            want = TC.taps_planes(P, nch)[0] + bias.astype(np.float64)[:, None, None]
            if regime == "onehot":
                assert set(np.unique(want).tolist()) == {0.0, 1.0} and 0 < int(want.sum()) <= 9 * nch
            assert np.array_equal(run_gather(lib, P, bias, zero, s, nch=nch).astype(np.float64), want), (regime, nch)
            if nch == 3:
                Q, seam = q_inputs(P)
                for mode in _modes(W):
                    assert np.array_equal(run_gather(lib, P, bias, zero, s, mode).astype(np.float64), want), (regime, mode)
                    assert np.array_equal(run_q(lib, Q, seam, bias, zero, s, mode).astype(np.float64), want), (regime, "q", mode)


def _all_entries(lib, s, regime, cr):
    """entry -> (got, taps, bias, center) of every tail entry at shape s."""
    out = {}
    for nch in (1, 2, 3):
        P, bias = TC.planes(regime, nch, s.H, s.W)
        center = TC.center_frame(cr, nch, s.h, s.w)
        out[f"nch {nch}"] = (run_gather(lib, P, bias, center, s, nch=nch), TC.taps_planes(P, nch), bias, center)
    out["gather"] = (run_gather(lib, P, bias, center, s), TC.taps_planes(P), bias, center)
    Q, seam = q_inputs(P)
    out["q"] = (run_q(lib, Q, seam, bias, center, s), TC.taps_q(Q, seam), bias, center)
    feat, wt, cb = TC.conv_inputs(regime if regime == "small" else "gauss", s.H, s.W)
    out["conv"] = (run_conv(lib, feat, wt, cb, center, s), TC.taps_conv(feat, wt), cb, center)
    return out


def test_constant_centre_frame(lib):
    """A constant centre frame stays the constant within the interpolation's bound at every pixel, the clamped rim included, whatever the
    index form."""
    for s in (TC.edge_shape(5, 33, (1.5, 1.3)), TC.edge_shape(2, 64, (4, 4)), TC.separating_shapes()[2]):
        for entry, (got, taps, bias, center) in _all_entries(lib, s, "small", "constant").items():
            const = center[:, :1, :1].astype(np.float64)
            assert bool((center == center[:, :1, :1]).all())
            r = TC.ratio(got, taps[0] + const, TC.bound(taps[1], taps[2], bias, np.abs(const) * np.ones_like(taps[0])))
            _note(entry, "small/constant", r)
            assert r <= 1.0, (s, entry, r)


def test_index_pin(lib):
    """At the three index-separating shapes, every entry, `uniform` and `checker` centre frames behind planes of 2^-10 (the bound is the
    residual's): the pairs of index forms under which an entry holds its bound at all of them are exactly one, the same for every entry."""
    held = {}
    for s in TC.separating_shapes():
        for cr in ("uniform", "checker"):
            for entry, (got, taps, bias, center) in _all_entries(lib, s, "small", cr).items():
                ok = _judged(entry, f"small/{cr}", got, taps, bias, center, s)
                held[entry] = held.get(entry, set(TC.FORM_PAIRS)) & ok
                print(f"{s} {cr:8s} {entry:7s} holds under {sorted(ok)}")
    print("index pin (row form, column form):", {e: sorted(v) for e, v in held.items()})
    assert all(len(v) == 1 for v in held.values()), held
    assert len({next(iter(v)) for v in held.values()}) == 1, held


@pytest.mark.parametrize("k", range(3))
def test_separating_shapes_full_matrix(lib, k):
    """Plane regimes x centre frames on the three gather entries at the index-separating shapes (several workgroups along y or x)."""
    s = TC.separating_shapes()[k]
    print(s, "gather", sorted(_check_gather(lib, s)), "nch", sorted(_check_nch(lib, s)), "q", sorted(_check_q(lib, s)))


def test_sharpness_on_the_kernels_outputs(lib):
    """Every mutant of tests/tail_cases.py used as the reference for the kernel's own output fails the bound under all four index forms;
    the unmutated reference holds under one."""
    for layout in ("p27", "nch", "q"):
        shape, P, bias, center = TC.mutant_inputs(layout)
        if layout == "q":
            got = run_q(lib, *q_inputs(P), bias, center, shape)
        else:
            got = run_gather(lib, P, bias, center, shape, nch=3 if layout == "nch" else None)
        assert TC.passing(TC.judge(got, TC.layout_taps(layout, P), bias, center, shape))
        for name, (layouts, _, _) in TC.MUTANTS.items():
            if layout not in layouts:
                continue
            cnt = []
            for fp in TC.FORM_PAIRS:
                bad, bnd = TC.mutant_reference(name, layout, P, bias, center, shape, *fp)
                cnt.append(int(TC.outside(got, bad, bnd).sum()))
            print(f"sharpness {layout:3s} {name:17s}: outside the bound at {min(cnt)} of {got.size} outputs")
            assert min(cnt) >= 1, (layout, name)


def test_refusals(lib):
    """A null pointer, a plane pitch below H * W, too few seam floats and nch outside 1 .. 3: a non-zero code and nothing launched (the
    output stays NaN)."""
    s = TC.edge_shape(5, 33, (1.5, 1.3))
    P, bias = TC.planes("gauss", 3, s.H, s.W)
    center = TC.center_frame("uniform", 3, s.h, s.w)
    Q, seam = q_inputs(P)
    feat, wt, cb = TC.conv_inputs("gauss", s.H, s.W)
    pb, pitch = _pitched(P, "vec")
    qb, _ = _pitched(Q, "vec")
    fb, _ = _pitched(feat, "vec")
    sb, bb, cbuf, wb = Buf(seam), Buf(bias), Buf(center), Buf(wt)
    out = Buf(n=3 * s.H * s.W)
    dims = (s.h, s.w, s.H, s.W)
    HW = s.H * s.W

    def gather(p=pb.ptr, pp=pitch, b=bb.ptr, c=cbuf.ptr, o=out.ptr):
        return lib.savsr_tail_gather(p, pp, b, c, *dims, o, None)

    def nch(p=pb.ptr, pp=pitch, n=3, b=bb.ptr, c=cbuf.ptr, o=out.ptr):
        return lib.savsr_tail_gather_nch(p, pp, n, b, c, *dims, o, None)

    def q(p=qb.ptr, pp=pitch, sm=sb.ptr, sf=seam.size, b=bb.ptr, c=cbuf.ptr, o=out.ptr):
        return lib.savsr_tail_gather_q(p, pp, sm, sf, b, c, *dims, o, None)

    def conv(p=fb.ptr, pp=pitch, w=wb.ptr, b=bb.ptr, c=cbuf.ptr, o=out.ptr):
        return lib.savsr_tail_residual(p, pp, w, b, c, *dims, o, None)

    for fn, ptrs in ((gather, "pbco"), (nch, "pbco"), (q, ("p", "sm", "b", "c", "o")), (conv, "pwbco")):
        for name in ptrs:
            assert fn(**{name: None}) != 0, (fn.__name__, name)
        assert fn(pp=HW - 1) != 0, fn.__name__
    assert q(sf=seam.size - 1) != 0
    assert nch(n=0) != 0 and nch(n=4) != 0
    assert out.untouched()
    assert gather() == 0 and np.isfinite(out.get()).all()                # (the same arguments unmutated do launch)


@pytest.mark.parametrize("c,h,w", TC.MASK_SHAPES)
def test_mask_branch(lib, c, h, w):
    """savsr_avgpool2 and savsr_upsample2x, channel-last, against float64 (pool: three additions and an exact x 0.25; upsample: lambda in
    {0, 0.25, 0.75}, the index exact in both forms).  16 x 130 x 128 upsamples to 1 064 960 outputs, more than 4096 workgroups of 256: the
    grid-stride loop; the pool takes it at 64 x 260 x 256."""
    shapes = [(c, h, w)] + ([(64, 260, 256)] if c * h * w > 2 ** 17 else [])
    for c, h, w in shapes:
        for regime, x in (("gauss", np.random.RandomState(c + h).standard_normal((h, w, c))),
                          ("decades", np.random.RandomState(c + w).standard_normal((h, w, c)) * 2.0 ** np.random.RandomState(3).uniform(-12, 12, (h, w, c)))):
            x = x.astype(F32)
            xb = Buf(x)
            if (c, h, w) != (64, 260, 256):
                up = Buf(n=4 * h * w * c)
                assert lib.savsr_upsample2x(xb.ptr, up.ptr, c, h, w, None) == 0
                ref, b = TC.upsample2x_reference(x)
                r = TC.ratio(up.get().reshape(2 * h, 2 * w, c), ref, b)
                _note("upsample2x", regime, r)
                assert r <= 1.0, (c, h, w, regime, r)
            po = Buf(n=(h // 2) * (w // 2) * c)
            assert lib.savsr_avgpool2(xb.ptr, po.ptr, c, h, w, None) == 0
            ref, b = TC.avgpool2_reference(x)
            r = TC.ratio(po.get().reshape(h // 2, w // 2, c), ref, b)
            _note("avgpool2", regime, r)
            assert r <= 1.0, (c, h, w, regime, r)
