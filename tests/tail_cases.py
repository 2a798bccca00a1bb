"""The kernels that write every frame -- savsr_tail_gather, savsr_tail_gather_nch, savsr_tail_gather_q, savsr_tail_residual (tail.hip,
satu_nf.hip) -- and the OSAdapt mask branch's savsr_avgpool2 / savsr_upsample2x (elementwise.hip): float64 references, the bilinear
source index in both of its fp32 forms, derived per-output bounds, inputs, shapes and mutants.  numpy and float64 only, no GPU import.

What a tail kernel computes per output (o, Y, X), in its own order:

    acc = 0;  acc += term_1; ...; acc += term_n      the taps: P[3 (3 ky + kx) + o][Y + ky - 1][X + kx - 1] (27-plane form), P[nch (3 ky + kx)
                                                     + o][..] (nch form), ky outer and kx inner, taps outside the image skipped; or (q form) per
                                                     ky: Q[3 ky + o][Y + ky - 1][X], then seam[Y + ky - 1][X >> 5][0][3 ky + o] where X % 32 == 0
                                                     and X > 0, or seam[..][1][..] where X % 32 == 31 and X + 1 < W; or (savsr_tail_residual)
                                                     576 FMAs acc = fma(w[o][c][ky][kx], feat[c][..], acc), c outer, then ky, then kx
    t   = acc + bias[o]
    top = (1 - lx) c[y0][x0] + lx c[y0][x1];  bot = (1 - lx) c[y1][x0] + lx c[y1][x1];  r = (1 - ly) top + ly bot
    out = t + r

The source index.  s = scale * (dst + 0.5f) - 0.5f with scale = fl32(fl32(in) / fl32(out)) is one line of C++ that the compiler may
contract into one FMA (`fused`: ONE rounding of the exact value) or leave as a product and a sum (`plain`: fl32(fl32(scale * d) - 0.5)).
`fused` is evaluated here in float64 and rounded once; that float64 evaluation is exact: d = dst + 0.5 has at most 14 significant bits
(dst < 8192), fl32(scale) has 24, so the product has at most 38 and the difference to 0.5 still fits float64's 53.  The two forms differ
by one ulp of s where they differ at all (2^-16 once s >= 128), i.e. by ulp(s) times the centre frame's local gradient in the output.
What follows s is reproduced as the kernels do it: s clamped below at 0, i0 = min(int(s), in - 1), i1 = i0 + (i0 < in - 1), lambda =
min(max(s - i0, 0), 1) (s - i0 is exact in fp32).  With the clamp of s in front, lambda's own clamp never acts: s <= in - 0.5 - scale / 2
< in for every in, out >= 1, so int(s) <= in - 1 and 0 <= s - i0 < 1 (`lambda_is_inside` checks it).  A kernel without fminf / fmaxf
alone computes the same function; the mutant `lambda_unclamped` below is the one that can be wrong, lambda taken from the unclamped s.

The residual reference interpolates in float64 with the fp32 indices and lambdas of a chosen form per axis (four combinations, FORM_PAIRS),
R, and the same interpolation of |center|, Rm.  Addresses are the kernels' flat ones, (o h + y) w + x, so that an index past a row or a
plane reads what the kernel would read (the next row, the next plane, OOB behind the last).

The bound (u = 2^-24 = U24 of tests/satu_cases.py, fp32's unit roundoff; nothing measured enters).  Every fp32 operation rounds its exact
result x to x (1 + d), |d| <= u; a term that passes k roundings on its way into the output carries at most gamma(k) = k u / (1 - k u) of
its magnitude.  The k per step:

  taps      n     n additions into an accumulator that starts at 0 (the first, 0 + x, is exact; it is counted all the same): n <= 9 in
                  the plane forms (3 x 3 taps, fewer on the rim), n <= 6 in the q form (per tap row Q and at most one seam: a pixel is
                  not both the first and the last of its segment), n = 576 FMAs in savsr_tail_residual (one rounding each; the staged
                  zeros of the padding add exactly)
  bias      1     t = acc + bias
  interp    6     1 - lx rounds (1), its product (1), the sum with lx c (1) -- the same three once more along y.  The kernels write each
                  level as fmaf(1 - l, a, l * b) (lerp_fma, common.hpp): 1 - l, l * b and the FMA round, 3 per level as well; the
                  uncontracted count covers that and any other contraction of `a * b + c`, which only drops a product's rounding
  final     1     out = t + r

so, with S = the sum of |term| over the n terms the kernel adds at this output (for the FMAs: |w| |feat|),

    |got - exact| <= gamma(n + 2) S + gamma(2) |bias| + gamma(7) Rm           (<= (n + 2) u (S + |bias| + Rm), as good as)

per output.  Underflow plays no part: every operand of the cases below is an exact zero or above 2^-40 in magnitude.

The mask branch (channel-last [h][w][c]):  avgpool2 = ((p00 + p01) + p10) + p11 (3 additions) times 0.25 (exact): gamma(3) * 0.25 * sum
|p|.  upsample2x: scale = 0.5, s = 0.5 dst - 0.25 is exact in both forms (one reference), lambda in {0, 0.25, 0.75} and 1 - lambda are
exact; each level rounds its products and its sum: gamma(4) Rm.

Plane values are multiples of 2^-30 below 2^17: every float64 sum of them is exact in any order, which is what lets the q form's
reference (`build_q`: row sums inside the 32-pixel segments, the two crossing terms per segment border in the seam) equal the 27-plane
reference of the same P bit for bit.
"""
import numpy as np

from tests.satu_cases import U24

F32 = np.float32
FORMS = ("plain", "fused")
FORM_PAIRS = tuple((fy, fx) for fy in FORMS for fx in FORMS)          # (rows, columns)
OOB = 1000.0                                                         # what a read behind the last plane of the centre frame finds
K_BIAS, K_INTERP, K_FINAL = 1, 6, 1
K_POOL, K_UP = 3, 4
PLANE_REGIMES = ("gauss", "decades", "altsign")                      # judged against the bound
EXACT_REGIMES = ("integers", "onehot")                               # bit for bit
CENTER_REGIMES = ("uniform", "checker", "decades", "constant")

# (h, w, scale): rows / columns whose index differs between the forms: 7 / 0, 0 / 6, 3 / 2
SEPARATING = ((200, 6, (3.9, 2)), (6, 200, (2, 3.7)), (150, 130, (1.3, 1.1)))
EDGE_W = (1, 3, 4, 8, 12, 31, 32, 33, 64, 65, 260)                   # no / one interior vector thread, W % 4, seam at x + 1 == W, partial segment, 2nd workgroup
EDGE_H = (1, 2, 5)
SMALL_SCALES = ((1.5, 1.3), (2.95, 3.75), (4, 4))
ONEHOT_SHAPES = ((12, 33), (10, 64))                                 # (H, W) that hold 27 impulses 3 pixels apart


def gamma(k):
    return k * U24 / (1.0 - k * U24)


def _d(v):
    return np.asarray(v, dtype=np.float64)


class Shape:
    """LR size h x w, HR size H x W, the nominal scale factors (only the `recip_scale` mutant reads them)."""

    def __init__(self, h, w, H, W, sc):
        self.h, self.w, self.H, self.W, self.sc = int(h), int(w), int(H), int(W), (float(sc[0]), float(sc[1]))

    def __repr__(self):
        return f"{self.h}x{self.w}->{self.H}x{self.W}"


def separating_shapes():
    return [Shape(h, w, round(h * sc[0]), round(w * sc[1]), sc) for h, w, sc in SEPARATING]


def edge_shape(H, W, sc):
    """The LR frame a scale factor sc would have blown up to about H x W (at least one pixel)."""
    return Shape(max(1, round(H / sc[0])), max(1, round(W / sc[1])), H, W, sc)


def edge_shapes(W):
    """Every edge height with edge width W, the small scales taken in turn."""
    k = EDGE_W.index(W)
    return [edge_shape(H, W, SMALL_SCALES[(k + i) % 3]) for i, H in enumerate(EDGE_H)]


# ----------------------------------------------------------------------------- source index
def scale32(n_in: int, n_out: int) -> np.float32:
    return F32(F32(n_in) / F32(n_out))


def source_index(n_out: int, scale, form: str) -> np.ndarray:
    """s [n_out] in fp32, unclamped, in the `plain` or the `fused` form (module docstring)."""
    d = np.arange(n_out, dtype=np.float64) + 0.5
    if form == "plain":
        t = (F32(scale) * d.astype(F32)).astype(F32)
        return (t - F32(0.5)).astype(F32)
    assert form == "fused"
    return (float(F32(scale)) * d - 0.5).astype(F32)


class Axis:
    """i0, i1 (int64) and lam (fp32) of one axis, as the kernels derive them from s."""

    def __init__(self, n_out, n_in, form, scale=None, align=False, clamp_i1=True, clamp_low=True):
        if align:                                                                  # mutant: align_corners=True
            sc = F32((n_in - 1) / (n_out - 1)) if n_out > 1 else F32(0)
            raw = (sc * np.arange(n_out, dtype=F32)).astype(F32)
        else:
            raw = source_index(n_out, scale32(n_in, n_out) if scale is None else scale, form)
        s = np.maximum(raw, F32(0))
        self.s = s
        self.i0 = np.minimum(s.astype(np.int64), n_in - 1)
        self.i1 = self.i0 + ((self.i0 < n_in - 1).astype(np.int64) if clamp_i1 else 1)
        self.unclipped = (s - self.i0.astype(F32)).astype(F32)
        self.lam = np.clip(self.unclipped, F32(0), F32(1))
        if not clamp_low:                                                          # mutant: lambda of the unclamped s, no fminf / fmaxf
            self.lam = (raw - self.i0.astype(F32)).astype(F32)


def lambda_is_inside(n_out: int, n_in: int) -> bool:
    return all(bool(((a.unclipped >= 0) & (a.unclipped < 1)).all()) and bool((a.s.astype(np.int64) <= n_in - 1).all())
               for a in (Axis(n_out, n_in, f) for f in FORMS))


def index_differences(n_out: int, n_in: int) -> int:
    """Output coordinates at which the two forms give another s."""
    sc = scale32(n_in, n_out)
    return int((source_index(n_out, sc, "plain") != source_index(n_out, sc, "fused")).sum())


def _axes(shape: Shape, fy, fx, recip_scale=False, align=False, clamp_i1=True, clamp_low=True):
    kw = dict(align=align, clamp_i1=clamp_i1, clamp_low=clamp_low)
    sy = F32(1) / F32(shape.sc[0]) if recip_scale else None
    sx = F32(1) / F32(shape.sc[1]) if recip_scale else None
    return Axis(shape.H, shape.h, fy, sy, **kw), Axis(shape.W, shape.w, fx, sx, **kw)


def residual(center, shape: Shape, fy: str, fx: str, **mut):
    """(R, Rm) [c][H][W] float64: the bilinear residual of center [c][h][w] with the fp32 indices and lambdas of forms (fy, fx), and the
    same interpolation of |center| (with |weights|).  mut: the index mutants of `_axes`."""
    c = np.asarray(center, F32)
    nch, h, w = c.shape
    ay, ax = _axes(shape, fy, fx, **mut)
    flat = np.concatenate([_d(c).reshape(-1), np.full(w + 2, OOB)])
    base = (np.arange(nch) * h * w)[:, None, None]

    def at(iy, ix):
        return base + (iy * w)[None, :, None] + ix[None, None, :]
    ly, lx = _d(ay.lam)[None, :, None], _d(ax.lam)[None, None, :]
    out = []
    for v in (flat, np.abs(flat)):
        f = np.abs if v is not flat else (lambda t: t)
        top = f(1 - lx) * v[at(ay.i0, ax.i0)] + f(lx) * v[at(ay.i0, ax.i1)]
        bot = f(1 - lx) * v[at(ay.i1, ax.i0)] + f(lx) * v[at(ay.i1, ax.i1)]
        out.append(f(1 - ly) * top + f(ly) * bot)
    return out[0], out[1]


# ----------------------------------------------------------------------------- taps
def _rim_count(n: int) -> np.ndarray:
    """Taps of a 3-tap axis that fall inside an axis of n pixels, per position."""
    i = np.arange(n)
    return 3 - (i == 0) - (i == n - 1)


def taps_planes(P, nch: int = 3, transposed=False, pad_clamp=False):
    """(A, S, n) [nch][H][W]: the nine shifted taps of P[nch (3 ky + kx) + o] in float64 (zero outside the image), the sum of their
    magnitudes and the number of taps the kernel adds.  nch = 3 is the 27-plane form.  Mutants: `transposed` P[nch (3 kx + ky) + o];
    `pad_clamp` the clamped pixel where the padding is."""
    P = _d(P)
    assert P.shape[0] == 9 * nch
    H, W = P.shape[1:]
    Pp = np.pad(P, ((0, 0), (1, 1), (1, 1)), mode="edge" if pad_clamp else "constant")
    A, S = np.zeros((nch, H, W)), np.zeros((nch, H, W))
    for ky in range(3):
        for kx in range(3):
            for o in range(nch):
                t = Pp[nch * ((3 * kx + ky) if transposed else (3 * ky + kx)) + o, ky:ky + H, kx:kx + W]
                A[o] += t
                S[o] += np.abs(t)
    n = np.broadcast_to((_rim_count(H)[:, None] * _rim_count(W)[None, :])[None], A.shape)
    return A, S, n


def seam_floats(H: int, W: int) -> int:
    return H * ((W + 31) // 32) * 18


def build_q(P):
    """27 planes P [27][H][W] -> (Q [9][H][W], seam [H][nseg][2][9]) in float64: Q[3 ky + o] = the three horizontal taps of tap row ky that
    stay inside the pixel's 32-pixel segment (and the image); seam[Y][seg][0][g] = what the first pixel of segment seg still needs from its
    left neighbour, seam[Y][seg][1][g] = what its last pixel needs from its right neighbour.  Entries the kernel must not read are NaN:
    side 0 of segment 0, side 1 where the segment's last pixel is the row's last or the segment is partial."""
    P = _d(P)
    H, W = P.shape[1:]
    nseg = (W + 31) // 32
    x = np.arange(W)
    Q, seam = np.zeros((9, H, W)), np.full((H, nseg, 2, 9), np.nan)
    for ky in range(3):
        for o in range(3):
            g = 3 * ky + o
            left, mid, right = (P[3 * (3 * ky + kx) + o] for kx in range(3))
            Q[g] = mid
            inl = (x % 32 != 0)
            Q[g][:, inl] += left[:, x[inl] - 1]
            inr = (x % 32 != 31) & (x + 1 < W)
            Q[g][:, inr] += right[:, x[inr] + 1]
            for seg in range(nseg):
                if seg > 0:
                    seam[:, seg, 0, g] = left[:, 32 * seg - 1]
                if 32 * seg + 32 < W:
                    seam[:, seg, 1, g] = right[:, 32 * seg + 32]
    return Q, seam


def taps_q(Q, seam, seam_at_x0=False, right_at_edge=False, swap=False):
    """(A, S, n) [3][H][W] of the q form: Q[3 ky + o][Y + ky - 1][X] plus the seams, as the kernel addresses them.  Mutants: the left
    seam added at x == 0 too; the right seam added at x + 1 == W too; the two sides swapped.  (A NaN that a mutant reads stays a NaN.)"""
    Q, seam = _d(Q), _d(seam)
    H, W = Q.shape[1:]
    x = np.arange(W)
    first = (x % 32 == 0) & ((x > 0) | seam_at_x0)
    last = (x % 32 == 31) & ((x + 1 < W) | right_at_edge)
    row, mag, cnt = np.zeros((9, H, W)), np.zeros((9, H, W)), np.zeros((H, W), np.int64)
    for g in range(9):
        row[g], mag[g] = Q[g], np.abs(Q[g])
        for sel, side in ((first, 0), (last, 1)):
            v = seam[:, x[sel] >> 5, side ^ int(swap), g]
            row[g][:, sel] += v
            mag[g][:, sel] += np.abs(v)
    cnt[:] = 1 + (first | last)[None, :]
    A, S, n = np.zeros((3, H, W)), np.zeros((3, H, W)), np.zeros((3, H, W), np.int64)
    z, zi = np.zeros((1, W)), np.zeros((1, W), np.int64)
    for ky in range(3):
        for o in range(3):
            g = 3 * ky + o
            for dst, src, pad in ((A, row[g], z), (S, mag[g], z), (n, cnt, zi)):
                dst[o] += np.concatenate([pad, src, pad])[ky:ky + H]
    return A, S, n


def taps_conv(feat, wt):
    """(A, S, n) [3][H][W] of savsr_tail_residual's 64 -> 3 conv: feat [64][H][W], wt [3][64][3][3]; S = |wt| * |feat|; n = 576."""
    feat, wt = _d(feat), _d(wt)
    H, W = feat.shape[1:]
    fp = np.pad(feat, ((0, 0), (1, 1), (1, 1)))
    A, S = np.zeros((3, H, W)), np.zeros((3, H, W))
    for ky in range(3):
        for kx in range(3):
            win = fp[:, ky:ky + H, kx:kx + W]
            A += np.einsum("oc,chw->ohw", wt[:, :, ky, kx], win)
            S += np.einsum("oc,chw->ohw", np.abs(wt[:, :, ky, kx]), np.abs(win))
    return A, S, np.full(A.shape, 576)


# ----------------------------------------------------------------------------- bound and verdicts
def bound(S, n, bias, Rm):
    b = np.abs(_d(bias))[:, None, None]
    return gamma(n + K_BIAS + K_FINAL) * S + gamma(K_BIAS + K_FINAL) * b + gamma(K_INTERP + K_FINAL) * Rm


def exact_and_bound(taps, bias, center, shape: Shape, fy, fx, bias_next=False, **mut):
    """taps = (A, S, n).  Mutant `bias_next`: the bias of channel (o + 1) % nch."""
    A, S, n = taps
    R, Rm = residual(center, shape, fy, fx, **mut)
    b = _d(bias)
    return A + (np.roll(b, -1) if bias_next else b)[:, None, None] + R, bound(S, n, bias, Rm)


def ratio(got, exact, bnd) -> float:
    """max |got - exact| / bound (0 / 0 counts as 0; a NaN or an error over a zero bound as inf)."""
    err = np.abs(_d(got) - exact)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / bnd)
    return float(np.inf) if bool(np.isnan(r).any()) else float(r.max())


def judge(got, taps, bias, center, shape: Shape, **mut) -> dict:
    """(fy, fx) -> worst |got - exact| / bound under that pair of index forms.  A launch passes where one of them is <= 1."""
    return {fp: ratio(got, *exact_and_bound(taps, bias, center, shape, *fp, **mut)) for fp in FORM_PAIRS}


def passing(verdict: dict) -> frozenset:
    return frozenset(fp for fp, r in verdict.items() if r <= 1.0)


def outside(a, exact, bnd) -> np.ndarray:
    """Outputs at which a is NOT within bnd of exact (a NaN on either side counts as outside)."""
    return ~(np.abs(_d(a) - exact) <= bnd)


# ----------------------------------------------------------------------------- inputs
def _rng(*seed):
    return np.random.RandomState([int(s) for s in seed])


def _grid(a) -> np.ndarray:
    """Rounded to multiples of 2^-30 (module docstring), then to fp32 (which keeps a multiple of 2^-30 one: either the value has 24 bits
    or fewer and stays, or its fp32 ulp is above 2^-30)."""
    a = np.round(_d(a) * 2.0 ** 30) / 2.0 ** 30
    assert float(np.abs(a).max(initial=0.0)) < 2.0 ** 17
    return a.astype(F32)


def onehot_positions(nplanes: int, H: int, W: int, seed: int = 0):
    """One (y, x) per plane on a grid of stride 3 that starts on the rim, in a shuffled order."""
    pos = [(y, x) for y in range(0, H, 3) for x in range(0, W, 3)]
    assert len(pos) >= nplanes, "shape too small for one impulse per plane"
    order = _rng(17, seed).permutation(len(pos))[:nplanes]
    return [pos[i] for i in order]


def planes(regime: str, nch: int, H: int, W: int, seed: int = 0):
    """(P [9 nch][H][W], bias [nch]) fp32.  gauss: N(0, 1).  decades: plane p times 2^e_p, e_p uniform in [-12, 12].  altsign: tap t =
    a_t * 64 + 2^-10 N(0, 1), a = (1, -1, 1, -1, 0, -1, 1, -1, 1): the taps cancel to 2^-16 of their magnitude sum.  integers: integers in
    [-8, 8], integer bias.  onehot: one 1.0 per plane (onehot_positions), bias 0.  small: gauss / 1024 with bias 0 (the index pin: the
    taps run, the bound is the residual's)."""
    g = _rng(3, PLANE_REGIMES.index(regime) if regime in PLANE_REGIMES else 9, nch, H, W, seed)
    n = 9 * nch
    bias = g.standard_normal(nch) * 0.5
    if regime == "gauss":
        P = g.standard_normal((n, H, W))
    elif regime == "small":
        P, bias = g.standard_normal((n, H, W)) / 1024, np.zeros(nch)
    elif regime == "decades":
        P = g.standard_normal((n, H, W)) * 2.0 ** g.uniform(-12, 12, (n, 1, 1))
    elif regime == "altsign":
        a = np.asarray([1, -1, 1, -1, 0, -1, 1, -1, 1], np.float64)[np.arange(n) // nch]
        P = a[:, None, None] * 64 + g.standard_normal((n, H, W)) / 1024
    elif regime == "integers":
        P, bias = g.randint(-8, 9, (n, H, W)), g.randint(-4, 5, nch)
    elif regime == "onehot":
        P, bias = np.zeros((n, H, W)), np.zeros(nch)
        for p, (y, x) in enumerate(onehot_positions(n, H, W, seed)):
            P[p, y, x] = 1.0
    else:
        raise ValueError(regime)
    return _grid(P), _grid(bias)


def center_frame(regime: str, nch: int, h: int, w: int, seed: int = 0) -> np.ndarray:
    """[nch][h][w] fp32.  uniform: [0, 1).  checker: 0 / 1 alternating (the largest gradient).  decades: N(0, 1) times 2^e per pixel, e
    uniform in [-12, 12].  constant: one value per channel.  zero: the exact regimes' centre frame."""
    g = _rng(5, h, w, nch, seed)
    if regime == "uniform":
        c = g.uniform(0, 1, (nch, h, w))
    elif regime == "checker":
        c = (np.arange(nch)[:, None, None] + np.arange(h)[None, :, None] + np.arange(w)[None, None, :]) % 2
    elif regime == "decades":
        c = g.standard_normal((nch, h, w)) * 2.0 ** g.uniform(-12, 12, (nch, h, w))
    elif regime == "constant":
        c = np.broadcast_to(np.asarray([0.7, -1.3, 0.1])[:nch, None, None], (nch, h, w))
    elif regime == "zero":
        c = np.zeros((nch, h, w))
    else:
        raise ValueError(regime)
    return np.ascontiguousarray(c, dtype=np.float64).astype(F32)


def conv_inputs(regime: str, H: int, W: int, seed: int = 0):
    """(feat [64][H][W], wt [3][64][3][3], bias [3]) fp32 for savsr_tail_residual.  gauss: N(0, 1) features, N(0, 1) / 24 weights.  decades:
    channel c of both times 2^e_c.  integers: small integers (every partial sum below 2^24: bit for bit).  onehot: channel c is one 1.0 at
    (3 (c // 8) + 1, 3 (c % 8) + 1), bias 0: out[o][y - ky + 1][x - kx + 1] = wt[o][c][ky][kx] exactly.  small: gauss features / 1024."""
    g = _rng(7, H, W, seed)
    feat, wt, bias = g.standard_normal((64, H, W)), g.standard_normal((3, 64, 3, 3)) / 24, g.standard_normal(3) * 0.5
    if regime == "decades":
        feat, wt = feat * 2.0 ** g.uniform(-12, 12, (64, 1, 1)), wt * 2.0 ** g.uniform(-12, 12, (1, 64, 1, 1))
    elif regime == "small":
        feat, bias = feat / 1024, np.zeros(3)
    elif regime == "integers":
        feat, wt, bias = g.randint(-8, 9, (64, H, W)), g.randint(-4, 5, (3, 64, 3, 3)), g.randint(-4, 5, 3)
    elif regime == "onehot":
        assert H >= 23 and W >= 23
        feat, bias = np.zeros((64, H, W)), np.zeros(3)
        for c in range(64):
            feat[c, 3 * (c // 8) + 1, 3 * (c % 8) + 1] = 1.0
    elif regime != "gauss":
        raise ValueError(regime)
    return feat.astype(F32), wt.astype(F32), bias.astype(F32)


def onehot_conv_expected(wt, H: int, W: int) -> np.ndarray:
    out = np.zeros((3, H, W), F32)
    for c in range(64):
        y, x = 3 * (c // 8) + 1, 3 * (c % 8) + 1
        for ky in range(3):
            for kx in range(3):
                out[:, y - ky + 1, x - kx + 1] = wt[:, c, ky, kx]
    return out


# ----------------------------------------------------------------------------- mutants
# name -> (the layouts it applies to, where in the reference it acts, its switch).  Each is ONE plausible kernel error.
MUTANTS = {
    "recip_scale":      (("p27", "nch", "q"), "index", dict(recip_scale=True)),       # 1 / fl32(scale_factor) in place of h / H
    "align_corners":    (("p27", "nch", "q"), "index", dict(align=True)),
    "i1_unclamped":     (("p27", "nch", "q"), "index", dict(clamp_i1=False)),         # reads the next row / plane on the last row / column
    "lambda_unclamped": (("p27", "nch", "q"), "index", dict(clamp_low=False)),        # extrapolates on the first row / column
    "taps_transposed":  (("p27", "nch"), "taps", dict(transposed=True)),
    "pad_clamp":        (("p27", "nch"), "taps", dict(pad_clamp=True)),
    "bias_next":        (("p27", "nch", "q"), "bias", dict(bias_next=True)),
    "seam_at_x0":       (("q",), "taps", dict(seam_at_x0=True)),
    "seam_right_edge":  (("q",), "taps", dict(right_at_edge=True)),                   # (needs W % 32 == 0)
    "seam_swapped":     (("q",), "taps", dict(swap=True)),
}
MUTANT_SHAPE = (5, 64, (1.5, 1.3))                                                    # H, W, scale: two full segments, the last ends the row


def mutant_inputs(layout: str, nch: int = 3):
    """The inputs every mutant is judged on, on the CPU and on the kernel's output: (shape, P, bias, center)."""
    shape = edge_shape(*MUTANT_SHAPE)
    P, bias = planes("gauss", nch, shape.H, shape.W, 41)
    return shape, P, bias, center_frame("uniform", nch, shape.h, shape.w, 41)


def layout_taps(layout: str, P, nch: int = 3, **mut):
    if layout == "q":
        Q, seam = build_q(P)
        return taps_q(Q.astype(F32), seam.astype(F32), **mut)
    return taps_planes(P, nch, **mut)


def mutant_reference(name: str, layout: str, P, bias, center, shape: Shape, fy, fx, nch: int = 3):
    """(the mutant's output, the CORRECT reference's bound)."""
    layouts, where, kw = MUTANTS[name]
    assert layout in layouts
    good = exact_and_bound(layout_taps(layout, P, nch), bias, center, shape, fy, fx)
    taps = layout_taps(layout, P, nch, **(kw if where == "taps" else {}))
    out, _ = exact_and_bound(taps, bias, center, shape, fy, fx, **(kw if where != "taps" else {}))
    return out, good[1]


# ----------------------------------------------------------------------------- mask branch
MASK_SHAPES = ((4, 2, 2), (4, 8, 10), (16, 8, 10), (64, 8, 10), (16, 130, 128))     # (c, h, w); the last: more than 4096 x 256 outputs


def avgpool2_reference(x):
    """x [h][w][c] -> (exact, bound) [h/2][w/2][c]."""
    x = _d(x)
    p = [x[dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)]
    return 0.25 * (p[0] + p[1] + p[2] + p[3]), gamma(K_POOL) * 0.25 * sum(np.abs(q) for q in p)


def upsample2x_reference(x):
    """x [h][w][c] -> (exact, bound) [2h][2w][c]: F.interpolate(scale_factor=2, bilinear, align_corners=False)."""
    x = _d(x)
    h, w, _ = x.shape
    ay, ax = Axis(2 * h, h, "fused", F32(0.5)), Axis(2 * w, w, "fused", F32(0.5))
    for a, n in ((ay, h), (ax, w)):
        assert bool((source_index(2 * n, F32(0.5), "plain") == source_index(2 * n, F32(0.5), "fused")).all())
        assert set(np.unique(a.lam).tolist()) <= {0.0, 0.25, 0.75}
    ly, lx = _d(ay.lam)[:, None, None], _d(ax.lam)[None, :, None]
    out = []
    for v in (x, np.abs(x)):
        top = (1 - lx) * v[ay.i0][:, ax.i0] + lx * v[ay.i0][:, ax.i1]
        bot = (1 - lx) * v[ay.i1][:, ax.i0] + lx * v[ay.i1][:, ax.i1]
        out.append((1 - ly) * top + ly * bot)
    return out[0], gamma(K_UP) * out[1]
