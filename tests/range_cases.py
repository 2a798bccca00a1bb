"""Dynamic-range regimes for the split-bf16 conv kernels, and CPU emulations of the kernels' arithmetic (numpy + torch, no GPU).

`regimes` yields activations and weights whose magnitudes differ by decades between channels, or whose outputs are dominated by a few
terms; `direct_emulation` / `wy_emulation` evaluate the convolution exactly as conv_mfma.hip / conv_wy.hip state their arithmetic --
every fp32 operand v as hi = bf16(v) (RNE), lo = bf16(v - hi), every product as hi hi + hi lo + lo hi -- but with the sums in float64, so
what separates a kernel from its emulation is fp32 accumulation alone.  Every bound of tests/test_range_cases.py and
tests/test_gpu_conv_range.py is PER OUTPUT ELEMENT and relative to that element's own S = sum |x| |w| (direct form) or S_wy = |A^T| applied
to sum |V| |U| (Winograd F(2,3) along y).

Worst case of the split, per product: |v - hi| <= 2^-8 |v|, |v - hi - lo| <= 2^-16 |v|, so
x w - (x_hi w_hi + x_hi w_lo + x_lo w_hi) = x_lo w_lo + r_x w + x r_w - (second order), |.| <= 3 * 2^-16 |x| |w|.
"""
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

REGIMES = ("gauss", "decades", "matched", "mean50", "vsmooth", "altsign", "sparse", "heavy", "addressed")
U17 = 2.0 ** -17                 # the unit the printed ratios are quoted in
SPLIT_WORST = 3 * 2.0 ** -16     # analytic worst case of one split product, relative to |x| |w|
BOUND_EXACT = 2.0 ** -14         # the GPU tests' bound against the exact value: SPLIT_WORST = 0.75 of it, the rest is fp32 accumulation
T_ACC_CPU = 2e-6                 # "accumulation order only", per output, of S (KBOUND of tests/test_gpu_precision.py): ATen's fp32 sums meet it
T_ACC = 1.5 * 2.22e-6            # the same for the GPU kernels: 1.5 x the worst measured ratio (direct form, `addressed` 320 -> 64: its 16 dominant
                                 # terms enter in the first 8 of 20 K chunks, the 324 accumulator updates of the other 12 then round at their scale); every
                                 # other (regime, shape, form) measured <= 1.7e-6, and 2^-17 = 7.6e-6 would be a finding, not a tolerance
SPARSE_HOLE = (slice(1, 5), slice(2, 7))      # rows 1 .. 4, columns 2 .. 6 of the `sparse` regime are zero in every channel


def _f32(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def slot_of(co, cin: int, ks: int):
    """(16-channel K chunk, tap) that dominates output channel co in the `addressed` regime."""
    taps = ks * ks
    s = co % ((cin // 16) * taps)
    return s // taps, s % taps


def regimes(cin: int, cout: int, ks: int, h: int, w: int, seed: int, only=None):
    """Yields (name, x [cin, h, w] fp32, wt [cout, cin, ks, ks] fp32) for every regime of REGIMES (or those named in `only`); a regime's
    draw depends on (seed, its name) only."""
    fan = cin * ks * ks
    for i, name in enumerate(REGIMES):
        if only is not None and name not in only:
            continue
        g = np.random.RandomState([seed, i])
        x = g.standard_normal((cin, h, w))
        wt = g.standard_normal((cout, cin, ks, ks)) / np.sqrt(fan)
        if name in ("decades", "matched"):
            sx = 10.0 ** g.uniform(-3, 3, cin)
            x = x * sx[:, None, None]
            if name == "decades":
                wt = wt * (10.0 ** g.uniform(-3, 3, cout))[:, None, None, None] * (10.0 ** g.uniform(-3, 3, cin))[None, :, None, None]
            else:
                wt = wt / sx[None, :, None, None]
        elif name == "mean50":
            x = 50.0 + x
        elif name == "vsmooth":
            x = g.standard_normal((cin, 1, w)) + 1e-3 * x
        elif name == "altsign":
            x = np.broadcast_to(g.uniform(0.1, 1.0, (1, h, w)), (cin, h, w))
            mag = np.abs(g.standard_normal((cout, 1, ks, ks))) / np.sqrt(fan) * (1.0 + 0.01 * g.standard_normal((1, cin, 1, 1)))
            wt = mag * np.where(np.arange(cin) % 2 == 0, 1.0, -1.0)[None, :, None, None]
        elif name == "sparse":
            x = x * (g.uniform(0, 1, (cin, h, w)) < 0.05)
            x[(slice(None),) + SPARSE_HOLE] = 0.0          # a hole wide enough for outputs with S == 0 (and S_wy == 0 for the row pair at y = 2)
        elif name == "heavy":
            x = np.clip(g.standard_cauchy((cin, h, w)), -1e4, 1e4)
        elif name == "addressed":
            chunk, tap = slot_of(np.arange(cout), cin, ks)
            own = (np.arange(cin)[None, :, None] // 16 == chunk[:, None, None]) & (np.arange(ks * ks)[None, None, :] == tap[:, None, None])
            wt = g.standard_normal((cout, cin, ks, ks)) / 4.0 * np.where(own, 1.0, 1e-4).reshape(cout, cin, ks, ks)
        yield name, _f32(x), _f32(wt)


def split(v: torch.Tensor):
    """fp32 v -> (hi, lo) as fp32 tensors holding bf16 values: hi = bf16(v), lo = bf16(v - hi), RNE both (packing.split_bf16_image)."""
    hi = v.to(torch.bfloat16).to(torch.float32)
    lo = (v - hi).to(torch.bfloat16).to(torch.float32)
    return hi, lo


def _conv(x, wt, pad):
    return F.conv2d(x[None].double(), wt.double(), None, padding=pad)[0]


def _conv3(xh, xl, wh, wl, pad, acc32: bool):
    """x_hi w_hi + x_hi w_lo + x_lo w_hi as ONE convolution over 3 cin channels: float64, or fp32 accumulation by ATen."""
    xs, ws = torch.cat([xh, xh, xl], 0), torch.cat([wh, wl, wh], 1)
    if acc32:
        return F.conv2d(xs[None], ws, None, padding=pad)[0].double()
    return _conv(xs, ws, pad)


def direct_emulation(x, wt, ks: int, drop=None, acc32: bool = False):
    """The direct form.  Returns a dict of [cout, h, w] float64 tensors: `exact` (float64 conv of the fp32 operands), `emul` (float64 sum of
    the three split products), `S` (conv of |x| and |w|), and with acc32 `acc32` (the three products accumulated in fp32 by ATen).
    drop = (chunk, tap): the simulated defect, x_lo w_hi missing for the 16 input channels of `chunk` at `tap`."""
    pad = ks // 2
    xh, xl = split(x)
    wh, wl = split(wt)
    out = dict(exact=_conv(x, wt, pad), emul=_conv3(xh, xl, wh, wl, pad, False), S=_conv(x.abs(), wt.abs(), pad))
    if acc32:
        out["acc32"] = _conv3(xh, xl, wh, wl, pad, True)
    if drop is not None:
        chunk, tap = drop
        wd = torch.zeros_like(wh)
        wd[:, 16 * chunk:16 * chunk + 16, tap // ks, tap % ks] = wh[:, 16 * chunk:16 * chunk + 16, tap // ks, tap % ks]
        out["emul"] = out["emul"] - _conv(xl, wd, pad)
    return out


WY_TAPS_OF_POS = ((0,), (0, 1, 2), (0, 1, 2), (2,))      # tap rows ky that enter U_pos (packing._wy_transform)


def wy_emulation(x, wt, drop=None, acc32: bool = False):
    """The Winograd F(2,3)-along-y form, structured as tests/test_gpu_precision.py::_wy_reference: row pairs start at even Y and read rows
    Y-1 .. Y+2 (zero outside the image); V is formed in fp32, U is packing.wy_transform_f64(wt) rounded to fp32; both are split, the three
    products summed in float64, then the output transform.  Returns `emul` and `S_wy` ([cout, h, w] float64; S_wy = |A^T| applied to the
    per-position sum |V| |U|), with acc32 also `acc32` (fp32 accumulation and fp32 output transform).
    drop = (chunk, pos, kx): the simulated defect, the lo half of U zero for the 16 input channels of `chunk` at (pos, kx)."""
    from savsr_amd.packing import wy_transform_f64
    cin, h, w = x.shape
    cout = wt.shape[0]
    npair = (h + 1) // 2
    xp = torch.zeros(cin, 2 * npair + 2, w)
    xp[:, 1:h + 1] = x
    d = [xp[:, i:i + 2 * npair:2] for i in range(4)]                   # rows Y-1 .. Y+2 of every pair: [cin, npair, w] each, fp32
    v = [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]           # fp32 arithmetic, as the staging
    u = torch.from_numpy(wy_transform_f64(wt).astype(np.float32))      # [4 pos][cout][cin][3 kx]: float64 U rounded once to fp32
    m, a, m32 = [], [], []
    for i in range(4):
        ui = u[i].unsqueeze(2)                                         # [cout][cin][1][3]
        vh, vl = split(v[i])
        uh, ul = split(ui)
        if drop is not None and drop[1] == i:
            ul = ul.clone()
            ul[:, 16 * drop[0]:16 * drop[0] + 16, :, drop[2]] = 0.0
        m.append(_conv3(vh, vl, uh, ul, (0, 1), False))
        a.append(_conv(v[i].abs(), ui.abs(), (0, 1)))
        if acc32:
            m32.append(_conv3(vh, vl, uh, ul, (0, 1), True).float())
    rows = lambda r0, r1: torch.stack([r0, r1], 2).reshape(cout, 2 * npair, w)[:, :h]      # noqa: E731
    out = dict(emul=rows(m[0] + m[1] + m[2], m[1] - m[2] - m[3]), S_wy=rows(a[0] + a[1] + a[2], a[1] + a[2] + a[3]))
    if acc32:
        out["acc32"] = rows(m32[0] + m32[1] + m32[2], m32[1] - m32[2] - m32[3]).double()
    return out


@lru_cache(maxsize=None)
def case(cin: int, cout: int, ks: int, h: int, w: int, regime: str, wy: bool = False):
    """One (shape, regime) with its emulations, computed once per process and shared (callers must not modify it): x, wt and the keys of
    direct_emulation; with wy also emul_wy and S_wy."""
    (_, x, wt), = regimes(cin, cout, ks, h, w, seed=cin * 7 + cout + h, only=(regime,))
    c = dict(x=x, wt=wt, **direct_emulation(x, wt, ks))
    if wy:
        e = wy_emulation(x, wt)
        c["emul_wy"], c["S_wy"] = e["emul"], e["S_wy"]
    return c


def ratio(err: torch.Tensor, s: torch.Tensor) -> float:
    """max over the outputs with s > 0 of err / s (0 if there are none)."""
    m = s > 0
    return float((err[m] / s[m]).max()) if bool(m.any()) else 0.0


# ----------------------------------------------------------------------------- the precision mode "fp16": regimes and emulations
# The fp16 forms of the same kernels (savsr_conv2d_batch_f16) round every operand ONCE to fp16 (RNE, subnormals kept, +-inf from 65520) and
# multiply exactly on the fp16 matrix cores; tests/test_range_cases_f16.py and tests/test_gpu_conv_range_f16.py hold them to per-output bounds
# as above.  fp16 has 5 exponent bits: the +-3 decades of `decades` leave its range, so F16_REGIMES carries `decades16` in its place, and three
# regimes at the range's ends -- `w_sub` / `x_sub` (every weight / activation fp16-subnormal, outputs of magnitude ~1) and `edge` (values at and
# beyond 65504 planted in Gaussian data: the only regime with non-finite outputs).
F16_NEW = ("decades16", "w_sub", "x_sub", "edge")
F16_REGIMES = tuple("decades16" if r == "decades" else r for r in REGIMES) + F16_NEW[1:]
F16_FINITE = F16_REGIMES[:-1]
F16_MIN_NORMAL = 2.0 ** -14
F16_INF_FROM = 65520.0           # the smallest magnitude RNE takes to infinity (65504 + half an ulp of 32)

# `edge`: (what, input channel, ((row, column, value), ...)); rows 4 / 5 are the two output rows of one Winograd row pair, 2 / 3 of another,
# 1 / 3 are d0 and d2 of the pair at 2, 7 / 8 lie in different pairs.  A plant is made where all its rows and its column are interior.
EDGE_PLANTS = (("65504", 0, ((2, 3, 65504.0),)), ("65519", 1, ((2, 7, 65519.0),)), ("65520", 2, ((2, 11, 65520.0),)),
               ("-70000", 3, ((2, 15, -70000.0),)), ("pair ++", 4, ((4, 19, 40000.0), (5, 19, 40000.0))),
               ("pair +-", 5, ((2, 23, 40000.0), (3, 23, -40000.0))), ("d0 - d2", 6, ((1, 27, 40000.0), (3, 27, -40000.0))),
               ("across pairs", 7, ((7, 31, 40000.0), (8, 31, 40000.0))))


def edge_plants(h: int, w: int, skip=()):
    """The plants of EDGE_PLANTS that fit a h x w image (every row <= h - 2, column <= w - 2), less those named in `skip`."""
    return [p for p in EDGE_PLANTS if p[0] not in skip and all(r <= h - 2 and c <= w - 2 for r, c, _ in p[2])]


def regimes_f16(cin: int, cout: int, ks: int, h: int, w: int, seed: int, only=None, skip_plants=()):
    """`regimes` for F16_REGIMES: the eight shared regimes are the SAME draws; a new regime's draw depends on (seed, its name) only."""
    fan = cin * ks * ks
    for name in F16_REGIMES:
        if only is not None and name not in only:
            continue
        if name in REGIMES:
            yield from regimes(cin, cout, ks, h, w, seed, only=(name,))
            continue
        g = np.random.RandomState([seed, len(REGIMES) + F16_NEW.index(name)])
        x = g.standard_normal((cin, h, w))
        wt = g.standard_normal((cout, cin, ks, ks))
        if name == "decades16":
            x = x * (10.0 ** g.uniform(-2, 2, cin))[:, None, None]
            wt = wt / np.sqrt(fan) * (10.0 ** g.uniform(-1.5, 1.5, cout))[:, None, None, None] * (10.0 ** g.uniform(-1.5, 1.5, cin))[None, :, None, None]
        elif name == "w_sub":
            x, wt = x * 2.0 ** 10, wt * 2.0 ** -17
        elif name == "x_sub":
            x, wt = x * 2.0 ** -17, wt * 2.0 ** 10
        else:
            wt = wt / np.sqrt(fan)
            for _, ch, pts in edge_plants(h, w, skip_plants):
                for r, c, v in pts:
                    x[ch, r, c] = v
        yield name, _f32(x), _f32(wt)


def f16_round(v, flush: bool = False) -> np.ndarray:
    """float64 array of fp16(v): numpy's RNE straight from float64 (packing._f16_image), subnormals kept, +-inf from 65520.  flush: results below
    2^-14 become zero instead (what a matrix core that does not take subnormal operands would compute with)."""
    with np.errstate(over="ignore"):
        r = np.asarray(v, dtype=np.float64).astype(np.float16).astype(np.float64)
    return np.where(np.abs(r) < F16_MIN_NORMAL, 0.0, r) if flush else r


def f16_toward_zero(v) -> np.ndarray:
    """fp16 array of v rounded TOWARD ZERO (the sharpness tests' defect): where RNE rounded away from zero, one fp16 step back."""
    v = np.asarray(v, dtype=np.float64)
    r = v.astype(np.float16)
    return np.where(np.abs(r.astype(np.float64)) > np.abs(v), np.nextafter(r, np.float16(0)), r)


def _r16(t: torch.Tensor, flush: bool = False) -> torch.Tensor:
    return torch.from_numpy(f16_round(t.double().numpy(), flush))


def f16_err(v: torch.Tensor) -> torch.Tensor:
    """e(v) >= |fp16(v) - v|: 2^-11 |v| in the normal range, 2^-25 (half a subnormal step) below 2^-14; 0 from 65520 on, where fp16(v) is
    an infinity and no bound is claimed."""
    a = v.double().abs()
    return torch.where(a < F16_MIN_NORMAL, torch.full_like(a, 2.0 ** -25), torch.where(a < F16_INF_FROM, 2.0 ** -11 * a, torch.zeros_like(a)))


def _bound16(x, ex, wt, ew, pad):
    """conv(e(x), |w|) + conv(|x|, e(w)) + conv(e(x), e(w)) as one convolution."""
    return _conv(torch.cat([ex, x.double().abs(), ex], 0), torch.cat([wt.double().abs(), ew, ew], 1), pad)


def nonfinite_class(t: torch.Tensor) -> torch.Tensor:
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    return torch.isposinf(t).to(torch.int8) + 2 * torch.isneginf(t).to(torch.int8) + 3 * torch.isnan(t).to(torch.int8)


def f16_direct_emulation(x, wt, ks: int, acc32: bool = False, drop=None, flush: bool = False):
    """The direct form in the precision mode "fp16".  Returns [cout, h, w] float64 tensors: `exact` (float64 conv of the fp32 operands), `emul`
    (float64 conv of fp16(x), fp16(w)), `S` = conv(|x|, |w|), `S16` = conv(|fp16 x|, |fp16 w|), `B` (the derived bound on |emul - exact|, see
    f16_err) and with acc32 `acc32` (the same products accumulated in fp32 by ATen).
    drop = (chunk, tap): the simulated defect, fp16(w) rounded toward zero for the 16 input channels of `chunk` at `tap`.
    flush: subnormal fp16 operands taken as zero."""
    pad = ks // 2
    xh, wh = _r16(x, flush), _r16(wt, flush)
    if drop is not None:
        chunk, tap = drop
        sl = (slice(None), slice(16 * chunk, 16 * chunk + 16), tap // ks, tap % ks)
        wh[sl] = torch.from_numpy(f16_toward_zero(wt[sl].double().numpy()).astype(np.float64))
    out = dict(exact=_conv(x, wt, pad), emul=_conv(xh, wh, pad), S=_conv(x.abs(), wt.abs(), pad), S16=_conv(xh.abs(), wh.abs(), pad),
               B=_bound16(x, f16_err(x), wt, f16_err(wt), pad))
    if acc32:
        out["acc32"] = F.conv2d(xh.float()[None], wh.float(), None, padding=pad)[0].double()
    return out


def f16_wy_emulation(x, wt, acc32: bool = False, drop=None, flush: bool = False):
    """The Winograd F(2,3)-along-y form in the precision mode "fp16", structured as wy_emulation: V formed in fp32, then rounded to fp16;
    U = packing.wy_transform_f64(wt) rounded once to fp16; exact products, float64 sums, the output transform in float64.  Returns `emul`,
    `S_wy` (|A^T| applied to the per-position conv(|V|, |U|)), `S16_wy` (the same of the rounded operands), `B_wy` (|A^T| applied to the
    per-position bound of f16_direct_emulation on (V, U), plus 2^-23 S_wy for the fp32 rounding of V itself), `V_bad` ([4 pos, npair, w] bool:
    some channel's V of that position is not finite in fp16) and with acc32 `acc32` (fp32 accumulation and fp32 output transform).
    drop = (chunk, pos, kx): fp16(U) rounded toward zero for the 16 input channels of `chunk` at (pos, kx)."""
    from savsr_amd.packing import wy_transform_f64
    cin, h, w = x.shape
    cout = wt.shape[0]
    npair = (h + 1) // 2
    xp = torch.zeros(cin, 2 * npair + 2, w)
    xp[:, 1:h + 1] = x
    d = [xp[:, i:i + 2 * npair:2] for i in range(4)]                   # rows Y-1 .. Y+2 of every pair: [cin, npair, w] each, fp32
    v = [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]           # fp32 arithmetic, as the staging
    u = torch.from_numpy(wy_transform_f64(wt))                         # [4 pos][cout][cin][3 kx], float64
    m, a, a16, b, m32 = [], [], [], [], []
    for i in range(4):
        ui = u[i].unsqueeze(2)                                         # [cout][cin][1][3]
        vh, uh = _r16(v[i], flush), _r16(ui, flush)
        if drop is not None and drop[1] == i:
            sl = (slice(None), slice(16 * drop[0], 16 * drop[0] + 16), 0, drop[2])
            uh[sl] = torch.from_numpy(f16_toward_zero(ui[sl].numpy()).astype(np.float64))
        m.append(_conv(vh, uh, (0, 1)))
        a.append(_conv(v[i].abs(), ui.abs(), (0, 1)))
        a16.append(_conv(vh.abs(), uh.abs(), (0, 1)))
        b.append(_bound16(v[i], f16_err(v[i]), ui, f16_err(ui), (0, 1)))
        if acc32:
            m32.append(F.conv2d(vh.float()[None], uh.float(), None, padding=(0, 1))[0])
    rows = lambda r0, r1: torch.stack([r0, r1], 2).reshape(cout, 2 * npair, w)[:, :h]      # noqa: E731
    s_wy = rows(a[0] + a[1] + a[2], a[1] + a[2] + a[3])
    out = dict(emul=rows(m[0] + m[1] + m[2], m[1] - m[2] - m[3]), S_wy=s_wy, S16_wy=rows(a16[0] + a16[1] + a16[2], a16[1] + a16[2] + a16[3]),
               B_wy=rows(b[0] + b[1] + b[2], b[1] + b[2] + b[3]) + 2.0 ** -23 * s_wy,
               V_bad=torch.stack([(vi.abs() >= F16_INF_FROM).any(0) for vi in v]))
    if acc32:
        out["acc32"] = rows(m32[0] + m32[1] + m32[2], m32[1] - m32[2] - m32[3]).double()
    return out


@lru_cache(maxsize=None)
def case16(cin: int, cout: int, ks: int, h: int, w: int, regime: str, wy: bool = False):
    """`case` for the precision mode "fp16" (the same seeds): x, wt and the keys of f16_direct_emulation; with wy also emul_wy, S_wy, S16_wy,
    B_wy and V_bad.  Shared: callers must not modify it."""
    (_, x, wt), = regimes_f16(cin, cout, ks, h, w, seed=cin * 7 + cout + h, only=(regime,))
    c = dict(x=x, wt=wt, **f16_direct_emulation(x, wt, ks))
    if wy:
        e = f16_wy_emulation(x, wt)
        c.update(emul_wy=e["emul"], S_wy=e["S_wy"], S16_wy=e["S16_wy"], B_wy=e["B_wy"], V_bad=e["V_bad"])
    return c
