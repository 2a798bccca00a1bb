"""Weight sets, head sets, data regimes and float64 references for the SATU kernels (satu.hip: the tuned 64-wide forms "plain", "p27", "q";
satu_nf.hip: the width-generic form "nf"), stage by stage (numpy + torch, no GPU, no engine).  The record LRcat is observable between the LR
and the HR stage, so each stage is held to a PER-OUTPUT bound relative to that output's own magnitude sum S (tests/range_cases.py does the
same for the conv kernels); tests/test_satu_cases.py checks this module on the CPU, tests/test_gpu_satu_range.py holds the kernels to it.

Split products (range_cases): an fp32 v is hi = bf16(v), lo = bf16(v - hi); x w - (x_hi w_hi + x_hi w_lo + x_lo w_hi) is at most
3 * 2^-16 |x| |w|.  u = 2^-24 is the unit roundoff of fp32.

LR stage.  K = Wk st + bk (split product, K = C terms), sta = sum_tap LeakyReLU_0.1(K) x_rep (fp32 FMAs, 25 terms), A = Ta sta (split
product whose B operand is the fp32 accumulator sta re-split in registers), B = Tb x, C = Cstack x (split products).  Magnitude pipeline:
S_K = |Wk| |st| + |bk|, S_sta = sum_tap S_K |x_rep|, S_A = |Ta| S_sta, S_B = |Tb| |x|, S_C = |Cstack| |x|.
  * B, C: |got - exact| <= 2^-14 S (3 * 2^-16 = 0.75 of it, the rest is room for the fp32 accumulation of 64 terms) and
    |got - emul| <= range_cases.T_ACC S, emul the three split products summed in float64 (K = 64 here; T_ACC was set on K up to 2880).
  * A: |got - exact| <= 2^-13 S_A.  The split of (Wk, st) moves K by <= 3 * 2^-16 S_K; LeakyReLU is 1-Lipschitz, so sta moves by
    <= 3 * 2^-16 S_sta and A by <= 3 * 2^-16 S_A; the second split (Ta, sta) adds <= 3 * 2^-16 |Ta| |sta| <= 3 * 2^-16 S_A: 6 * 2^-16 = 0.75
    of 2^-13, the rest is fp32 accumulation (64 + 25 + 64 terms: ~153 u S_A = 0.07 of the bound) and the tuned kernels' LeakyReLU written as
    0.55 k + 0.45 |k| (fp32 constants: slope 0.55f - 0.45f = 0.1 (1 + 2.4e-7) on negative k, 2^-25 S_sta).
    No `emul` BOUND is given for this chained stage: the B operand of the second product is the kernel's own fp32 sta; an emulation's sta
    differs from it in its last bits (accumulation order), the re-split's lo half bf16(v - hi) then rounds differently, and the product moves
    by the same 2^-16 order as the split error itself -- there is no "accumulation only" residue to hold to T_ACC.  `emul` of A (float64
    sums, sta rounded once to fp32 before the re-split) exists for the defect simulations, which compare at 2^-13 S_A.
  * S == 0  =>  the output is 0 bit for bit (every term is a product with a zero factor).

HR stage.  out[p] = b[p] + G(B[p], off) + G(A[p], soff) + sum_{n,j} wbe[n][j][p] r_n z_j, z_j = sum_m r_m G(C[m][j], off), G the bilinear
gather with zeros padding at position ((gxn + (off 2) / (w - 1)) + 1) / 2 (w - 1).  S is the same expression on magnitudes; S4 is S
without b and with every tap weight of a gather replaced by 1 for the taps inside the image (the sensitivity to a weight error).
  * |got - exact| <= 2^-14 S + 2 delta_pos S4.  One split stage: (wbe, v = r_n z_j), v formed in fp32 (the tuned forms; the generic form
    multiplies in fp32, no split at all).  The gathers are fp32 FMAs of 4 taps, z of 16 terms.
  * delta_pos bounds the fp32 error of a sampling position against the float64 evaluation from the SAME fp32 inputs (table entry off, gxn),
    from make_taps' operations for a position inside [-1, w]: onx = fl(fl(2 off) / (w - 1)) errs by u |onx|; gx = fl(gxn + onx) by u |gx|;
    fl(gx + 1) by u |gx + 1|; / 2 is exact; the product with (w - 1) errs by u |ix|.  With |gxn| <= w / (w - 1) (base positions lie inside
    the image), |gx| <= (w + 1) / (w - 1), |gx + 1| <= 2 w / (w - 1) and |onx| <= |gx| + |gxn|:
        |ix_fp32 - ix| <= (w - 1) / 2 * u ((2 w + 1) + (w + 1) + 2 w) / (w - 1) + u w = u (3.5 w + 1).
    A bilinear weight is a product of two factors in [0, 1] with slope 1 in its axis: it errs by <= dx + dy, plus 2.5 u of its own
    arithmetic (1 - l: u / 2; the product: u; l = ix - floor(ix) is exact).  dx + dy + 2.5 u <= u (7 max(h, w) + 4.5) <= 8 u max(h, w)
    from max(h, w) >= 5 on.  So DELTA_POS = 4 u max(h, w) per axis, and an output errs by <= sum_k |dw_k| |v_k| <= 2 DELTA_POS S4.  Where the
    fp32 position falls on the other side of an integer than the float64 one, the kernel's taps are the neighbouring cell's: bilinear
    interpolation is continuous, the same bound holds with the neighbour's values, so S4 counts every tap column / row that a position
    within DELTA_POS of the float64 one can touch.
  * Exact: S == 0 => 0 bit for bit; every tap outside the image (`outside` heads) => the output is its fusion_b entry bit for bit.

Sharpness.  A slot (one (tap, channel group, k step) of kernel_conv, one k step of Wb or of wbe) that loses the lo half of its weights errs
by sum w_lo x_hi.  With random weights that is 0.1 .. 1.6 of the 2^-13 bound in the outputs the slot dominates (16 lo halves of random size
and sign, measured on the emulation): the bound would see it in some outputs and miss it in others.  The `addressed` set therefore builds
its dominant weights with a lo half of 0.6 .. 0.9 * 2^-9 of the value (_lo_rich) and `impulse` keeps st positive where it is O(1), so the
lost term is >= 2^-10 of the output's S.  The defect tests then assert: the bound fails in EVERY output whose S passes through the slot by
>= 1 - 10^-3 (`dominated`), and holds in every output whose S passes through it by <= 2^-7 (`untouched`: a lost lo half, <= 2^-8 of a term,
moves those by <= 2^-15 S); outputs in between are not asserted.
"""
from functools import lru_cache

import numpy as np
import torch

from savsr_amd.packing import acc_row, fold_satu_nf, row_q
from savsr_amd.utils import synth
from tests import range_cases as R

U24 = 2.0 ** -24
BOUND_B = 2.0 ** -14             # one split stage (B, C of the LR stage; the HR stage's expert product)
BOUND_A = 2.0 ** -13             # two chained split stages (A of the LR stage)
WEIGHT_SETS = ("synth", "wdecades", "negk", "addressed", "probe")
HEAD_SETS = ("mlp", "zero", "integer", "half", "straddle", "outside", "wide", "r_sat")
LR_REGIMES = ("gauss", "decades", "mean50", "vsmooth", "sparse", "heavy", "hole", "impulse")
HR_REGIMES = ("gauss", "decades", "mean50", "vsmooth", "sparse", "heavy")
HOLE = (slice(0, 6), slice(1, 7))               # `hole`: x is zero in rows 0 .. 5, columns 1 .. 6 of every channel (>= 5 x 5 with the replicate border)
LR_SHAPES = ((6, 7), (9, 33), (17, 40), (8, 31))
HR_SHAPES = ((9, 33, (4, 4)), (13, 18, (2.5, 3.5)), (7, 6, (1.5, 4)), (19, 23, (3.9, 3.9)))


def delta_pos(h: int, w: int) -> float:
    return 4 * U24 * max(h, w)


# ----------------------------------------------------------------------------- weight sets and head sets
@lru_cache(maxsize=None)
def _base(c: int):
    if c == 64:
        return synth.synth_state_dict(seed=0)
    from savsr_amd.archs.savsr_arch import SAVSR
    return synth.synth_state_dict(synth.manifest_of(SAVSR(num_feat=c).state_dict()), seed=0)


def _t(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def kconv_kstep(ch, tap, c: int):
    """`addressed`: the 16-channel k step of kernel_conv row 25 ch + tap that keeps O(1) weights."""
    return (ch + tap) % (c // 16)


def _lo_rich(g, shape) -> np.ndarray:
    """Positive values in [0.25, 0.75) whose bf16 split has a lo half of 0.6 .. 0.9 * 2^-9 of the value: hi (1 + 2^-9 t), hi a bf16 number with
    its mantissa in [1, 1.5) -- the offset stays below half a bf16 step (2^-8 of the binade), so hi is the split's hi.  The `addressed` set
    builds its dominant weights from them: a product that loses this lo half errs by >= 2^-10 of its magnitude, 8 (16) times the 2^-13
    (2^-14) bound, instead of by a random amount that can be small by chance."""
    hi = (1.0 + g.randint(0, 64, shape) / 128.0) * 2.0 ** g.randint(-2, 0, shape)
    return hi * (1.0 + 2.0 ** -9 * g.uniform(0.6, 0.9, shape))


def weights(name: str, c: int = 64) -> dict:
    """The state dict of weight set `name` at num_feat c: synth's with `upsample.*` entries edited."""
    sd = dict(_base(c))
    p = "upsample."
    g = np.random.RandomState([WEIGHT_SETS.index(name), c])
    dec = lambda n: 10.0 ** g.uniform(-2, 2, n)      # noqa: E731
    if name == "wdecades":
        sd[p + "kernel_conv.0.weight"] = sd[p + "kernel_conv.0.weight"] * _t(dec(25 * c)).view(-1, 1, 1, 1) * _t(dec(c)).view(1, -1, 1, 1)
        sd[p + "fusion.weight"] = sd[p + "fusion.weight"] * _t(dec(c)).view(-1, 1, 1, 1) * _t(dec(2 * c)).view(1, -1, 1, 1)
        sd[p + "weight_compress"] = sd[p + "weight_compress"] * _t(dec(c)).view(1, 1, -1, 1, 1)
        sd[p + "weight_expand"] = sd[p + "weight_expand"] * _t(dec(c)).view(1, -1, 1, 1, 1)
    elif name == "negk":
        sd[p + "kernel_conv.0.weight"] = sd[p + "kernel_conv.0.weight"] * 4.0
        sd[p + "kernel_conv.0.bias"] = sd[p + "kernel_conv.0.bias"] - 3.0
    elif name == "addressed":
        n = np.arange(25 * c)
        own = (np.arange(c)[None, :] // 16) == kconv_kstep(n // 25, n % 25, c)[:, None]
        sd[p + "kernel_conv.0.weight"] = _t(np.where(own, _lo_rich(g, (25 * c, c)), 1e-4 * g.standard_normal((25 * c, c)) / 4.0)).view(25 * c, c, 1, 1)
        sd[p + "kernel_conv.0.bias"] = sd[p + "kernel_conv.0.bias"] * 1e-4
        eye = lambda: (np.eye(c) * (1.0 + 1e-4 * g.uniform(1, 2, c) * g.choice([-1.0, 1.0], c))      # noqa: E731
                       + (1 - np.eye(c)) * 2.0 ** -12 * _lo_rich(g, (c, c)) * g.choice([-1.0, 1.0], (c, c)))      # (~1e-4, lo-rich as well)
        sd[p + "fusion.weight"] = _t(np.concatenate([eye(), eye()], 1)).view(c, 2 * c, 1, 1)
        sd[p + "fusion.bias"] = sd[p + "fusion.bias"] * 1e-4
        mj = np.arange(c // 2)                                            # compress row (m, j) = 8-wide at c = 64: one dominant input channel
        wc = 1e-4 * g.standard_normal((c // 2, c))
        wc[mj, (5 * mj + 3) % c] = _lo_rich(g, c // 2) * g.choice([-1.0, 1.0], c // 2)
        sd[p + "weight_compress"] = _t(wc).view(4, c // 8, c, 1, 1)
        we = 1e-4 * g.standard_normal((4, c, c // 8))                     # expand row co: one dominant (n, j)
        co = np.arange(c)
        we[co % 4, co, (co // 4) % (c // 8)] = _lo_rich(g, c) * g.choice([-1.0, 1.0], c)
        sd[p + "weight_expand"] = _t(we).view(4, c, c // 8, 1, 1)
    elif name == "probe":
        sd[p + "fusion.weight"] = _t(np.concatenate([np.zeros((c, c)), np.eye(c)], 1)).view(c, 2 * c, 1, 1)
        sd[p + "fusion.bias"] = torch.zeros(c)
        sd[p + "weight_expand"] = torch.zeros_like(sd[p + "weight_expand"])
    else:
        assert name == "synth", name
    return sd


def expand_dominant(co, c: int = 64):
    """`addressed`: the (n, j) that dominates row co of weight_expand."""
    return co % 4, (co // 4) % (c // 8)


def with_heads(sd: dict, name: str, h: int = 0, w: int = 0) -> dict:
    """sd with the coordinate MLP's heads of head set `name`.  A head weight of 0 with a bias gives the same offset / routing at every HR
    pixel; offsets are (x, y) pairs in LR pixels, `offset` for the gather of (B, C), `st_offset` for the gather of A."""
    sd = dict(sd)
    p = "upsample."

    def const(off, soff):
        for k, v in (("offset", off), ("st_offset", soff)):
            sd[p + k + ".weight"] = torch.zeros_like(sd[p + k + ".weight"])
            sd[p + k + ".bias"] = _t(np.array(v, dtype=np.float64))
    if name == "zero":
        const((0, 0), (0, 0))
    elif name == "integer":
        const((1, -2), (-1, 1))
    elif name == "half":
        const((0.5, -0.5), (-0.25, 0.75))
    elif name == "straddle":      # base positions span (-0.5, size - 0.5): -+0.4 puts the first / last HR columns and rows into (-1, 0) / (size - 1, size)
        const((-0.4, 0.4), (0.4, -0.4))
    elif name == "outside":
        assert h > 0 and w > 0
        const((w + 3, h + 3), (-(w + 3), -(h + 3)))
    elif name == "wide":
        for k in ("offset.weight", "st_offset.weight"):
            sd[p + k] = sd[p + k] * 6.0
    elif name == "r_sat":
        sd[p + "routing.0.weight"] = torch.zeros_like(sd[p + "routing.0.weight"])
        sd[p + "routing.0.bias"] = _t(np.array([20.0, -20.0, 20.0, -20.0]))
    else:
        assert name == "mlp", name
    return sd


# ----------------------------------------------------------------------------- data regimes
def st_kstep(y, x, c: int):
    """`impulse`: the 16-channel k step in which st is O(1) at pixel (y, x)."""
    return (-y - x) % (c // 16)


def impulse_positions(c: int, h: int, w: int):
    """`impulse`: (y, x) of channel ch's only nonzero pixel, y + x = -ch modulo c / 16 -- with kconv_kstep and st_kstep, EVERY tap of the 5 x 5
    window around it then meets its O(1) weights at a pixel whose O(1) st channels are the same k step (tap = 5 ky + kx = ky + kx modulo 4).
    Different channels get different pixels as far as the image has them."""
    nks = c // 16
    order = np.random.RandomState(7).permutation(h * w)
    by_class = [[(q // w, q % w) for q in order if (q // w + q % w) % nks == k] for k in range(nks)]
    used = [0] * nks
    pos = []
    for ch in range(c):
        k = (-ch) % nks
        pos.append(by_class[k][used[k] % len(by_class[k])])
        used[k] += 1
    return pos


def _gen(name: str, n: int, h: int, w: int, seed: int) -> np.ndarray:
    (_, x, _), = R.regimes(n, 1, 1, h, w, seed, only=(name,))
    return x.numpy().astype(np.float64)


@lru_cache(maxsize=None)
def lr_data(regime: str, c: int, h: int, w: int):
    """(x, st) [c, h, w] fp32 of an LR-stage regime; shared, callers must not modify them."""
    seed = 1000 * c + 37 * h + w
    g = np.random.RandomState([seed, LR_REGIMES.index(regime)])
    if regime in HR_REGIMES:
        x, st = _gen(regime, c, h, w, seed), _gen(regime, c, h, w, seed + 1)
    elif regime == "hole":
        x, st = _gen("sparse", c, h, w, seed), _gen("gauss", c, h, w, seed + 1)
        x = np.where(g.uniform(0, 1, x.shape) < 0.5, g.standard_normal(x.shape), x)      # denser than `sparse` outside the hole
        x[(slice(None),) + HOLE] = 0.0
    else:
        assert regime == "impulse", regime
        x = np.zeros((c, h, w))
        for ch, (y, xx) in enumerate(impulse_positions(c, h, w)):
            x[ch, y, xx] = g.uniform(0.5, 2.0) * g.choice([-1.0, 1.0])
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        own = (np.arange(c)[:, None, None] // 16) == st_kstep(yy, xx, c)[None]
        st = np.where(own, g.uniform(0.5, 1.5, (c, h, w)), 1e-4 * g.standard_normal((c, h, w)))      # (positive where O(1): with `addressed`, K = +S_K)
    return _t(x), _t(st)


@lru_cache(maxsize=None)
def ramp(c: int, h: int, w: int):
    """x of the `probe` weights: channel 0 = column index, 1 = row index, 2 = 1, 3 = a checkerboard of +-1, the rest 0 (all exact in bf16:
    the record's B part is x bit for bit); st Gaussian (A is multiplied by Wa = 0)."""
    x = np.zeros((c, h, w))
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    x[0], x[1], x[2], x[3] = xx, yy, 1.0, 1.0 - 2.0 * ((xx + yy) % 2)
    return _t(x), _t(np.random.RandomState(5).standard_normal((c, h, w)))


@lru_cache(maxsize=None)
def hr_record(regime: str, rec: int, h: int, w: int):
    """A record [h, w, rec] fp32 in an HR-stage regime, every float of it drawn (the form's layout decides what each one means); shared."""
    x = _gen(regime, rec, h, w, 500 * rec + 37 * h + w).transpose(1, 2, 0)
    return _t(x)


# ----------------------------------------------------------------------------- record layouts and folded matrices
def form_rows(form: str) -> int:
    return 64 if form == "plain" else 32


def record_perm(form: str, c: int) -> np.ndarray:
    """perm[i] = index into the stacked rows (A rows | B rows | C-stack) of record float i (satu.hip's header comment; satu_nf.hip's):
    (A | B) in MFMA accumulator order per lane half, 16 registers per 32-row tile, then the C-stack in natural order."""
    rows = form_rows(form)
    nb = rows // 32
    perm = np.empty(64 * nb + c // 2, dtype=np.int64)
    for hh in range(2):
        for t in range(nb):
            for r in range(16):
                row = 32 * t + acc_row(r, hh)
                perm[32 * nb * hh + 16 * t + r] = row
                perm[32 * nb * hh + 16 * nb + 16 * t + r] = rows + row
    perm[64 * nb:] = 2 * rows + np.arange(c // 2)
    return perm


def record_kind(form: str, c: int) -> np.ndarray:
    """0 / 1 / 2 for the record floats that hold A / B / C."""
    rows = form_rows(form)
    return np.minimum(record_perm(form, c) // rows, 2)


def folded(sd, c: int, form: str) -> dict:
    """fold_satu_nf's float64 matrices of `form`, each rounded to fp32 as the packers round them before the bf16 split (float64 arrays)."""
    m = fold_satu_nf(sd, c, row_q if form == "q" else None, tail=form != "plain")
    return {k: v.astype(np.float32).astype(np.float64) for k, v in m.items()}


def _split(a: np.ndarray):
    hi, lo = R.split(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
    return hi.double().numpy(), lo.double().numpy()


def _mm3(wh, wl, xh, xl):
    return wh @ xh + wh @ xl + wl @ xh


def _sta(k: np.ndarray, x: np.ndarray, c: int, h: int, w: int, lrelu: bool = True) -> np.ndarray:
    """sum_tap f(K[25 ch + tap]) x_rep[ch][y + ky - 2][x + kx - 2], tap = 5 ky + kx: [c, h w]."""
    k = (np.where(k > 0, k, 0.1 * k) if lrelu else k).reshape(c, 25, h, w)
    xp = np.pad(x.reshape(c, h, w), ((0, 0), (2, 2), (2, 2)), mode="edge")
    out = np.zeros((c, h, w))
    for ky in range(5):
        for kx in range(5):
            out += k[:, 5 * ky + kx] * xp[:, ky:ky + h, kx:kx + w]
    return out.reshape(c, h * w)


def lr_reference(sd, c: int, form: str, x: torch.Tensor, st: torch.Tensor, drop=None) -> dict:
    """The LR stage on x, st [c, h, w] fp32 in float64, per record element [h, w, rec] in `form`'s layout: `exact`, `S`, `emul` (see the module
    docstring; for A it carries no accumulation-only bound), `bound` (2^-13 S for A, 2^-14 S for B and C), `kind`; and the planes `sta`,
    `S_sta` [c, h, w].
    drop: the simulated defect in `emul`, ("kconv", tap, cg, ks): kernel_conv rows 25 (32 cg + i) + tap without the lo half of their weights in
    k step ks; ("wb", ks): Tb without its lo half in k step ks.  `S_slot` is then the part of S that passes through that slot."""
    m = folded(sd, c, form)
    h, w = x.shape[1:]
    x64, st64 = x.double().numpy().reshape(c, -1), st.double().numpy().reshape(c, -1)
    wk, bk, ta, tb, cs = m["kconv"], m["kconv_b"], m["ta"], m["tb"], m["cstack"]
    sta = _sta(wk @ st64 + bk[:, None], x64, c, h, w)
    s_k = np.abs(wk) @ np.abs(st64) + np.abs(bk)[:, None]
    s_sta = _sta(s_k, np.abs(x64), c, h, w, lrelu=False)
    # the emulation: every operand split, the three products summed in float64
    wkh, wkl = _split(wk)
    sth, stl = _split(st64)
    xh, xl = _split(x64)
    k_e = _mm3(wkh, wkl, sth, stl) + bk[:, None]
    s_slot = None
    if drop is not None and drop[0] == "kconv":
        _, tap, cg, ks = drop
        rows, cols = 25 * (32 * cg + np.arange(32)) + tap, slice(16 * ks, 16 * ks + 16)
        k_e[rows] -= wkl[rows][:, cols] @ sth[cols]
        sk1 = np.zeros_like(s_k)
        sk1[rows] = np.abs(wk[rows][:, cols]) @ np.abs(st64[cols])
        s_slot = [np.abs(ta) @ _sta(sk1, np.abs(x64), c, h, w, lrelu=False), np.zeros((len(tb), h * w)), np.zeros((len(cs), h * w))]
    sta_e = _sta(k_e, x64, c, h, w).astype(np.float32).astype(np.float64)
    tah, tal = _split(ta)
    tbh, tbl = _split(tb)
    csh, csl = _split(cs)
    sh, sl = _split(sta_e)
    a_e, b_e, c_e = _mm3(tah, tal, sh, sl), _mm3(tbh, tbl, xh, xl), _mm3(csh, csl, xh, xl)
    if drop is not None and drop[0] == "wb":
        cols = slice(16 * drop[1], 16 * drop[1] + 16)
        b_e = b_e - tbl[:, cols] @ xh[cols]
        s_slot = [np.zeros((len(ta), h * w)), np.abs(tb[:, cols]) @ np.abs(x64[cols]), np.zeros((len(cs), h * w))]
    perm = record_perm(form, c)
    rec = lambda a, b, cc: np.concatenate([a, b, cc], 0)[perm].T.reshape(h, w, -1)      # noqa: E731
    out = dict(exact=rec(ta @ sta, tb @ x64, cs @ x64), emul=rec(a_e, b_e, c_e),
               S=rec(np.abs(ta) @ s_sta, np.abs(tb) @ np.abs(x64), np.abs(cs) @ np.abs(x64)),
               kind=record_kind(form, c), sta=sta.reshape(c, h, w), S_sta=s_sta.reshape(c, h, w))
    out["bound"] = np.where(out["kind"] == 0, BOUND_A, BOUND_B) * out["S"]
    if s_slot is not None:
        out["S_slot"] = rec(*s_slot)
    return out


# ----------------------------------------------------------------------------- HR stage
def unique_axes(h: int, w: int, scale):
    """What a launch of the HR stage is given for (h, w, scale), as the engine computes it (launch.satu_axes): the distinct fp32 coor values
    and their index per HR row / column, the normalised base grid."""
    from savsr_amd.packing import get_hw, satu_axis_tables
    H, W = get_hw(h, w, scale)
    ch, _, gyn = satu_axis_tables(H, h, scale[0])
    cw, _, gxn = satu_axis_tables(W, w, scale[1])
    uh, ih = np.unique(ch, return_inverse=True)
    uw, iw = np.unique(cw, return_inverse=True)
    return dict(H=H, W=W, uh=uh.astype(np.float32), uw=uw.astype(np.float32), ih=ih.reshape(-1).astype(np.int32), iw=iw.reshape(-1).astype(np.int32),
                gyn=gyn.astype(np.float32), gxn=gxn.astype(np.float32))


def make_taps32(gxn, gyn, onx, ony, h: int, w: int) -> dict:
    """satu.hip's make_taps line for line in numpy fp32 (arrays broadcast against each other): x0, y0, dx, dy (int) and wgt [4, ...] (nw, ne,
    sw, se; fp32), plus the unclamped fp32 position ix, iy."""
    f = np.float32
    gxn, gyn, onx, ony = (np.asarray(a, dtype=f) for a in (gxn, gyn, onx, ony))
    fw1, fh1 = f(w - 1), f(h - 1)
    gx = gxn + onx
    gy = gyn + ony
    ix = ((gx + f(1)) / f(2)) * fw1
    iy = ((gy + f(1)) / f(2)) * fh1
    ix, iy = np.broadcast_arrays(ix, iy)
    raw = (ix.copy(), iy.copy())
    ix = np.minimum(np.maximum(ix, f(-2)), f(w) + f(1))
    iy = np.minimum(np.maximum(iy, f(-2)), f(h) + f(1))
    xw, yn = np.floor(ix), np.floor(iy)
    lx, ly = ix - xw, iy - yn
    ex, sy = f(1) - lx, f(1) - ly
    x0, y0 = xw.astype(np.int64), yn.astype(np.int64)
    z = f(0)
    wx0, wx1 = np.where((x0 >= 0) & (x0 < w), ex, z), np.where((x0 + 1 >= 0) & (x0 + 1 < w), lx, z)
    wy0, wy1 = np.where((y0 >= 0) & (y0 < h), sy, z), np.where((y0 + 1 >= 0) & (y0 + 1 < h), ly, z)
    cx0, cy0 = np.clip(x0, 0, w - 1), np.clip(y0, 0, h - 1)
    t = dict(x0=cx0, y0=cy0, dx=np.clip(x0 + 1, 0, w - 1) - cx0, dy=np.clip(y0 + 1, 0, h - 1) - cy0,
             wgt=np.stack([wy0 * wx0, wy0 * wx1, wy1 * wx0, wy1 * wx1]).astype(f), ix=raw[0], iy=raw[1])
    assert t["wgt"].dtype == f and lx.dtype == f
    return t


def _taps64(ix, iy, h: int, w: int) -> dict:
    """The same taps from float64 positions: clamped tap coordinates and float64 weights, 0 outside the image."""
    ix, iy = np.clip(ix, -2.0, w + 1.0), np.clip(iy, -2.0, h + 1.0)
    xw, yn = np.floor(ix), np.floor(iy)
    lx, ly = ix - xw, iy - yn
    x0, y0 = xw.astype(np.int64), yn.astype(np.int64)
    wx0, wx1 = np.where((x0 >= 0) & (x0 < w), 1 - lx, 0.0), np.where((x0 + 1 >= 0) & (x0 + 1 < w), lx, 0.0)
    wy0, wy1 = np.where((y0 >= 0) & (y0 < h), 1 - ly, 0.0), np.where((y0 + 1 >= 0) & (y0 + 1 < h), ly, 0.0)
    cx0, cy0 = np.clip(x0, 0, w - 1), np.clip(y0, 0, h - 1)
    return dict(x0=cx0, y0=cy0, dx=np.clip(x0 + 1, 0, w - 1) - cx0, dy=np.clip(y0 + 1, 0, h - 1) - cy0,
                wgt=np.stack([wy0 * wx0, wy0 * wx1, wy1 * wx0, wy1 * wx1]))


def _gather(planes: np.ndarray, t: dict, wgt=None) -> np.ndarray:
    """sum_k wgt[k] planes[:, y_k, x_k] -> [n, H, W] (float64)."""
    wgt = t["wgt"] if wgt is None else wgt
    out = 0.0
    for k in range(4):
        yy, xx = t["y0"] + (k >> 1) * t["dy"], t["x0"] + (k & 1) * t["dx"]
        out = out + wgt[k].astype(np.float64)[None] * planes[:, yy, xx]
    return out


def _reach(planes_abs: np.ndarray, ix, iy, h: int, w: int, d: float) -> np.ndarray:
    """sum of |planes| over every in-image tap that a position within d of (ix, iy) can touch (S4's gathers): columns floor(ix - d) ..
    floor(ix + d) + 1, rows alike."""
    ix, iy = np.clip(ix, -2.0, w + 1.0), np.clip(iy, -2.0, h + 1.0)
    xa, xb = np.floor(ix - d).astype(np.int64), np.floor(ix + d).astype(np.int64) + 1
    ya, yb = np.floor(iy - d).astype(np.int64), np.floor(iy + d).astype(np.int64) + 1
    assert int((xb - xa).max()) <= 2 and int((yb - ya).max()) <= 2
    out = 0.0
    for j in range(3):
        for i in range(3):
            yy, xx = ya + j, xa + i
            ok = (yy <= yb) & (xx <= xb) & (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            out = out + np.where(ok, 1.0, 0.0)[None] * planes_abs[:, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
    return out


def per_pixel_table(table: np.ndarray, ax: dict) -> np.ndarray:
    """[H, W, 8] fp32: table[ih[Y]][iw[X]] of a phase table [n_uh, n_uw, 8]."""
    return np.asarray(table, dtype=np.float32)[ax["ih"].astype(np.int64)][:, ax["iw"].astype(np.int64)]


def positions64(tab: np.ndarray, ax: dict, h: int, w: int, which: int):
    """Float64 sampling positions (ix, iy) [H, W] of gather `which` (0: off, 1: soff) from the fp32 table entries and the fp32 base grid."""
    t = tab.astype(np.float64)
    gx = ax["gxn"].astype(np.float64)[None, :] + t[..., 4 + 2 * which] * 2 / (w - 1)
    gy = ax["gyn"].astype(np.float64)[:, None] + t[..., 5 + 2 * which] * 2 / (h - 1)
    return (gx + 1) / 2 * (w - 1), (gy + 1) / 2 * (h - 1)


def taps32(tab: np.ndarray, ax: dict, h: int, w: int, which: int) -> dict:
    """make_taps32 for gather `which`, the offsets normalised in fp32 as the kernels normalise them: (off * 2) / (size - 1)."""
    f = np.float32
    onx, ony = (tab[..., 4 + 2 * which] * f(2)) / f(w - 1), (tab[..., 5 + 2 * which] * f(2)) / f(h - 1)
    return make_taps32(ax["gxn"][None, :], ax["gyn"][:, None], onx, ony, h, w)


def hr_reference(sd, c: int, form: str, rec: torch.Tensor, tab: np.ndarray, ax: dict, defect=None, emul: bool = False) -> dict:
    """The HR stage on a record [h, w, rec floats] fp32 with the per-pixel table `tab` [H, W, 8] fp32 (per_pixel_table), in float64:
    `exact`, `S`, `S4`, `bound` = 2^-14 S + 2 DELTA_POS S4, each [rows, H, W] in the form's row order (64, or 32 with the rows beyond 27 zero).
    emul (or a defect): also `emul` -- positions and tap weights from make_taps32, every fp32 product the kernels round (w_k r_m,
    r_n z_j) rounded, (wbe, v) split for the tuned forms, sums in float64.
    defect: ("wbe", ks): wbe without its lo half in k step ks (k = 8 n + j); ("shift",): the eastern taps of the `off` gather one column
    further east; ("nozero",): out-of-image taps keep their bilinear weight (and read the clamped pixel)."""
    m = folded(sd, c, form)
    h, w = rec.shape[:2]
    rows, J = form_rows(form), c // 8
    stacked = np.empty((2 * rows + c // 2, h, w))
    stacked[record_perm(form, c)] = rec.double().numpy().transpose(2, 0, 1)
    pa, pb, pc = stacked[:rows], stacked[rows:2 * rows], stacked[2 * rows:]
    t64 = tab.astype(np.float64)
    r = t64[..., :4].transpose(2, 0, 1)                                     # [4, H, W]
    wbe, fb = m["wbe"], m["fb"]                                             # [4 n][J j][rows], [rows]
    d = delta_pos(h, w)

    def evaluate(to, ts, pa_, pb_, pc_, rr, wbe_, fb_, tj_round=None):
        z = sum(rr[mi][None] * _gather(pc_[mi * J:(mi + 1) * J], to) for mi in range(4)) if tj_round is None else tj_round
        u = (rr[:, None] * z[None]).reshape(4 * J, *z.shape[1:])          # (n, j)
        return fb_[:, None, None] + _gather(pb_, to) + _gather(pa_, ts) + np.einsum("qp,qhw->phw", wbe_.reshape(4 * J, rows), u)
    po, ps = positions64(tab, ax, h, w, 0), positions64(tab, ax, h, w, 1)
    to, ts = _taps64(*po, h, w), _taps64(*ps, h, w)
    out = dict(exact=evaluate(to, ts, pa, pb, pc, r, wbe, fb), S=evaluate(to, ts, np.abs(pa), np.abs(pb), np.abs(pc), np.abs(r), np.abs(wbe), np.abs(fb)))
    zr = sum(np.abs(r[mi])[None] * _reach(np.abs(pc[mi * J:(mi + 1) * J]), *po, h, w, d) for mi in range(4))
    ur = (np.abs(r)[:, None] * zr[None]).reshape(4 * J, *zr.shape[1:])
    out["S4"] = _reach(np.abs(pb), *po, h, w, d) + _reach(np.abs(pa), *ps, h, w, d) + np.einsum("qp,qhw->phw", np.abs(wbe).reshape(4 * J, rows), ur)
    out["bound"] = BOUND_B * out["S"] + 2 * d * out["S4"]
    out["pos"] = (po, ps)
    if emul or defect is not None:
        f = np.float32
        eo, es = taps32(tab, ax, h, w, 0), taps32(tab, ax, h, w, 1)
        if defect is not None and defect[0] == "nozero":
            for t_ in (eo, es):
                ixc, iyc = np.clip(t_["ix"], f(-2), f(w + 1)), np.clip(t_["iy"], f(-2), f(h + 1))
                lx, ly = ixc - np.floor(ixc), iyc - np.floor(iyc)
                t_["wgt"] = np.stack([(1 - ly) * (1 - lx), (1 - ly) * lx, ly * (1 - lx), ly * lx]).astype(f)
        if defect is not None and defect[0] == "shift":
            nx0 = np.clip(eo["x0"] + 1, 0, w - 1)
            eo = dict(eo, x0=nx0, dx=np.clip(eo["x0"] + 1 + eo["dx"], 0, w - 1) - nx0)
        r32 = tab[..., :4].transpose(2, 0, 1)
        z = 0.0
        for mi in range(4):      # z_j = sum_k sum_m fl(w_k r_m) C[m][j](tap k)
            z = z + _gather(pc[mi * J:(mi + 1) * J], eo, wgt=(eo["wgt"] * r32[mi][None]).astype(f))
        v = (r32[:, None] * z.astype(f)[None]).astype(f).reshape(4 * J, *z.shape[1:]).astype(np.float64)      # fl(r_n fl(z_j))
        wq = wbe.reshape(4 * J, rows)
        if form == "nf":
            e = np.einsum("qp,qhw->phw", wq, v)
        else:
            vh, vl = _split(v)
            wh, wl = _split(wq)
            if defect is not None and defect[0] == "wbe":
                wl = wl.copy()
                wl[16 * defect[1]:16 * defect[1] + 16] = 0.0
                s_slot = np.einsum("qp,qhw->phw", np.abs(wq[16 * defect[1]:16 * defect[1] + 16]), np.abs(v[16 * defect[1]:16 * defect[1] + 16]))
                out["S_slot"] = s_slot
            e = sum(np.einsum("qp,qhw->phw", a, b) for a, b in ((wh, vh), (wh, vl), (wl, vh)))
        out["emul"] = fb[:, None, None] + _gather(pb, eo) + _gather(pa, es) + e
        out["taps32"] = (eo, es)
    return out


def worst(err: np.ndarray, s: np.ndarray) -> float:
    """max over the outputs with s > 0 of err / s (0 if there are none)."""
    msk = s > 0
    return float((err[msk] / s[msk]).max()) if bool(msk.any()) else 0.0
