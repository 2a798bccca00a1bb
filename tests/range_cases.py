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
