"""The conv kernels' EPILOGUE alone (bias, the four activations, per-pixel mask, two residuals with a scale, channel-slice store, fused
pool) against float64, per output element, for every activation with every operand subset, in every form of conv_mfma.hip and conv_wy.hip.

Each case runs the conv twice on the same inputs, weight image, algo and geometry: BARE (no bias, ACT_NONE, no mask, no residual; the stored
output is `a`) and with the epilogue E.  The reference is E applied in float64 to the STORED `a` (tests/epilogue_cases.py): the accumulation
is bit-identical between the two runs, the split-bf16 / fp16 product error cancels, and what is left are the epilogue's own few roundings.
The bound is derived there (u = 2^-24 times each rounded intermediate, propagated by the later steps' Lipschitz factors, FMA or not) and
no measured factor enters.  The output is a channel slice of a NaN-filled wider tensor and the guard channels are asserted; res1 and res2
are slices of NaN-filled wider tensors with pixel pitches of their own; every descriptor of a form's 96-entry matrix has operands of its own
and goes out in launches of savsr_conv2d_max_batch() convs, neighbours differing in activation and operands -- and once more alone, where
it must give the same bits (a descriptor field carried over from the previous tile's conv cannot hide in a batch of identical epilogues).

Measured on an MI355X (this file's own run, `pytest -s` prints the table at the end): worst |got - reference| / bound per form, activation
and operand subset (b bias, m mask, 1 res1, 2 res2; max over the form's shapes and regimes).  No bound was adjusted after the first run.  A
ratio of 1.00 is a single rounding at a half-ulp tie, which attains u |x|; 0.00 is an epilogue that rounds nothing (bit-exact).
  direct 16-row        ---- ---2 --1- --12 -m-- -m-2 -m1- -m12 b--- b--2 b-1- b-12 bm-- bm-2 bm1- bm12
    lrelu 0.2             .    .    .    .    .    .    .    .    .    .    .    .    .    .    . 0.93
    none                  .    .    .    .    .    .    . 0.94    .    .    .    .    .    .    .    .
    relu                  .    .    .    .    .    .    .    .    .    . 1.00    .    .    .    .    .
    sigmoid               .    .    .    . 0.55    .    .    .    .    .    .    .    .    .    .    .
  direct 1x1           ---- ---2 --1- --12 -m-- -m-2 -m1- -m12 b--- b--2 b-1- b-12 bm-- bm-2 bm1- bm12
    lrelu -0.25        0.00 0.99 1.00 0.96 0.99 0.97 0.99 0.88 1.00 0.95 0.98 0.94 0.95 0.82 0.96 0.83
    lrelu 0.2          0.95 0.98 1.00 0.93 1.00 0.95 0.99 0.90 1.00 0.97 0.98 0.90 0.93 0.85 0.95 0.81
    lrelu 1.5          1.00 0.99 1.00 0.93 0.99 0.97 0.99 0.89 0.87 0.89 0.99 0.80 0.86 0.83 0.95 0.90
    none               0.00 0.99 1.00 0.99 0.99 0.97 0.99 0.95 1.00 0.96 0.99 0.91 0.96 0.82 0.95 0.78
    relu               0.00 0.99 1.00 0.96 0.99 0.93 0.99 0.92 1.00 0.97 0.97 0.88 0.95 0.90 0.93 0.76
    sigmoid            0.49 0.54 0.99 0.83 0.55 0.50 0.99 0.92 0.37 0.47 0.97 0.64 0.42 0.49 0.95 0.86
  direct 3x3           ---- ---2 --1- --12 -m-- -m-2 -m1- -m12 b--- b--2 b-1- b-12 bm-- bm-2 bm1- bm12
    lrelu -0.25        0.00 1.00 1.00 0.96 1.00 0.96 0.99 0.90 1.00 0.93 0.98 0.92 0.95 0.85 0.98 0.89
    lrelu 0.2          0.95 0.99 1.00 0.95 1.00 0.96 0.99 0.95 1.00 0.96 1.00 0.89 0.98 0.84 0.97 0.90
    lrelu 1.5          1.00 0.99 1.00 0.97 1.00 0.93 0.99 0.89 0.87 0.84 0.99 0.84 0.87 0.77 0.95 0.84
    none               0.00 0.99 1.00 0.96 1.00 0.95 1.00 0.90 1.00 0.96 0.99 0.92 0.96 0.89 0.96 0.83
    relu               0.00 1.00 1.00 0.94 0.99 0.92 0.99 0.89 1.00 0.95 0.98 0.90 0.97 0.82 0.96 0.81
    sigmoid            0.49 0.57 0.99 0.92 0.58 0.52 0.99 0.85 0.39 0.48 0.98 0.55 0.46 0.49 0.97 0.80
  direct 3x3 fp16      ---- ---2 --1- --12 -m-- -m-2 -m1- -m12 b--- b--2 b-1- b-12 bm-- bm-2 bm1- bm12
    lrelu -0.25        0.00 1.00 1.00 0.96 1.00 0.95 0.99 0.85 1.00 0.93 0.99 0.88 0.92 0.90 0.98 0.85
    lrelu 0.2          0.95 0.99 1.00 0.95 0.99 0.95 0.99 0.88 1.00 0.96 1.00 0.92 0.94 0.82 0.98 0.92
    lrelu 1.5          1.00 0.99 1.00 0.95 1.00 0.93 0.99 0.90 0.87 0.84 0.96 0.82 0.84 0.74 0.99 0.83
    none               0.00 0.99 1.00 0.96 1.00 0.94 0.99 0.92 1.00 0.96 0.98 0.93 0.97 0.87 0.97 0.78
    relu               0.00 0.99 1.00 0.94 0.99 0.94 0.99 0.86 1.00 0.95 0.99 0.88 0.96 0.89 0.95 0.84
    sigmoid            0.49 0.51 0.99 0.84 0.58 0.52 0.99 0.88 0.39 0.48 0.98 0.54 0.43 0.49 0.97 0.80
  direct partial       ---- ---2 --1- --12 -m-- -m-2 -m1- -m12 b--- b--2 b-1- b-12 bm-- bm-2 bm1- bm12
    lrelu -0.25        0.00 0.98 1.00 0.88 0.97 0.94 0.98 0.83 1.00 0.85 0.94 0.82 0.93 0.78 0.94 0.68
    lrelu 0.2          0.95 0.98 1.00 0.92 0.99 0.94 0.96 0.84 0.99 0.93 0.96 0.87 0.93 0.74 0.90 0.79
    lrelu 1.5          1.00 0.97 1.00 0.88 0.98 0.95 0.99 0.78 0.86 0.80 0.96 0.77 0.80 0.67 0.91 0.70
    none               0.00 0.97 1.00 0.92 0.98 0.87 0.97 0.83 1.00 0.95 0.99 0.85 0.93 0.79 0.92 0.71
    relu               0.00 0.98 1.00 0.85 0.99 0.86 0.99 0.75 1.00 0.89 0.94 0.84 0.84 0.69 0.88 0.77
    sigmoid            0.48 0.48 0.94 0.82 0.55 0.48 0.97 0.70 0.36 0.45 0.90 0.48 0.40 0.46 0.91 0.79
  direct partial fp16  ---- ---2 --1- --12 -m-- -m-2 -m1- -m12 b--- b--2 b-1- b-12 bm-- bm-2 bm1- bm12
    lrelu -0.25        0.00 0.75 0.90 0.74 0.87 0.74 0.86 0.61 0.20 0.44 0.72 0.64 0.43 0.46 0.73 0.55
    lrelu 0.2          0.93 0.80 0.92 0.67 0.86 0.67 0.92 0.66 0.28 0.69 0.93 0.58 0.67 0.46 0.71 0.50
    lrelu 1.5          0.96 0.88 1.00 0.84 0.92 0.75 0.90 0.69 0.75 0.61 0.67 0.69 0.61 0.54 0.70 0.66
    none               0.00 0.91 0.98 0.73 0.95 0.75 0.87 0.74 1.00 0.66 0.90 0.64 0.68 0.55 0.88 0.53
    relu               0.00 0.97 0.93 0.57 0.93 0.84 0.82 0.65 0.84 0.46 0.75 0.55 0.76 0.49 0.56 0.48
    sigmoid            0.41 0.46 0.94 0.60 0.41 0.43 0.92 0.71 0.33 0.36 0.44 0.37 0.34 0.42 0.42 0.39
  winograd-y           ---- ---2 --1- --12 -m-- -m-2 -m1- -m12 b--- b--2 b-1- b-12 bm-- bm-2 bm1- bm12
    lrelu -0.25        0.00 0.99 1.00 0.95 1.00 0.95 0.99 0.93 1.00 0.97 0.99 0.94 0.95 0.88 0.99 0.85
    lrelu 0.2          0.95 0.99 1.00 0.96 1.00 0.96 0.99 0.94 1.00 0.96 1.00 0.93 0.94 0.87 0.98 0.90
    lrelu 1.5          1.00 1.00 1.00 0.95 1.00 0.96 0.99 0.89 0.87 0.88 0.99 0.86 0.88 0.81 0.98 0.82
    none               0.00 0.99 1.00 0.98 1.00 0.96 0.99 0.94 1.00 0.98 0.99 0.95 0.99 0.85 0.98 0.84
    relu               0.00 0.99 1.00 0.98 1.00 0.91 0.99 0.89 1.00 0.97 0.99 0.96 0.94 0.86 0.98 0.86
    sigmoid            0.49 0.56 0.99 0.92 0.61 0.55 0.99 0.87 0.39 0.48 0.97 0.62 0.48 0.49 0.96 0.81
  winograd-y fp16      ---- ---2 --1- --12 -m-- -m-2 -m1- -m12 b--- b--2 b-1- b-12 bm-- bm-2 bm1- bm12
    lrelu -0.25        0.00 0.99 1.00 0.96 1.00 0.94 1.00 0.93 1.00 0.97 1.00 0.92 0.94 0.86 1.00 0.89
    lrelu 0.2          0.95 0.99 1.00 0.96 1.00 0.98 0.99 0.90 1.00 0.96 0.99 0.92 0.96 0.88 0.98 0.89
    lrelu 1.5          1.00 0.99 1.00 0.96 1.00 0.95 0.99 0.92 0.87 0.87 0.99 0.88 0.91 0.84 0.96 0.84
    none               0.00 0.99 1.00 0.98 1.00 0.97 1.00 0.94 1.00 0.99 0.99 0.93 0.96 0.89 0.99 0.92
    relu               0.00 0.99 1.00 0.98 1.00 0.92 0.99 0.91 1.00 0.97 0.99 0.96 0.96 0.85 0.98 0.82
    sigmoid            0.49 0.55 0.99 0.89 0.57 0.58 0.99 0.90 0.37 0.48 0.97 0.62 0.45 0.49 0.96 0.81
  pool rows behind an epilogue: <= 2.65 * 2^-24 of the cell's sum |out| (bound 255 * 2^-24), both forms, both modes; the pooled ReLU conv
  alone (Winograd-y: the straight-line instantiation) gives the batch's output and pool bits; NaN guards left, right and behind intact.
  non-finite accumulators (fp16 `edge` plants and one -inf beside the +inf): +inf / -inf / NaN 571 / 598 / 175 of 25344 (direct 64 -> 64),
  138 / 144 / 54 of 3200 (64 -> 16), 5 / 13 / 3 of 200 (16 -> 1), 819 / 801 / 620 of 36992 (Winograd-y); classes as documented on every path.  With
  the partial-channel path's former fmaxf / select, ReLU gave 0 for -inf and NaN there and test_nonfinite_accumulators failed at 64 -> 16
  and 16 -> 1 (and passed in the interior and Winograd-y paths): conv_mfma.hip now runs the max form on that path too.
  sharpness, direct and Winograd-y alike: every mutant fails the bound on 99.8-100 % of the elements it can change, absent_bias_as_quad on
  67.8 % (where ReLU is zero before and after the wrong bias nothing changes).
"""
import copy

import numpy as np
import pytest
import torch

from tests import epilogue_cases as EC
from tests import range_cases as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# form -> shapes (cin, cout, ks, nsrc, h, w): the smallest that still have a last partial 32-column segment, rows below the image and more
# than one tile.  The first shape of a form, and 16 -> 1 at 10 x 12, also run the `large` and `mirror` scale regimes.
FORMS = {
    "direct 3x3":     [(64, 64, 3, 1, 12, 33), (128, 128, 3, 1, 12, 33)],                    # interior path; two output blocks
    "direct 1x1":     [(192, 64, 1, 3, 7, 50)],
    "direct partial": [(64, 16, 3, 1, 10, 12), (64, 16, 3, 1, 5, 6), (64, 8, 3, 1, 10, 12), (64, 8, 3, 1, 5, 6),
                       (16, 1, 3, 1, 10, 12), (16, 1, 3, 1, 5, 6)],                          # PXT == 1 && !chan_full: its own activation chain
    "winograd-y":     [(64, 64, 3, 1, 17, 34), (64, 64, 3, 1, 36, 70)],                      # WINOGRAD_Y (full tiles) and _THROUGHPUT (strips)
}
F16_FORMS = {"direct 3x3": FORMS["direct 3x3"][:1], "direct partial": FORMS["direct partial"][4:], "winograd-y": FORMS["winograd-y"]}


ALL_REGIMES = {(16, 1, 3, 1, 10, 12)}           # besides the first shape of every form: the scalar store / residual path of cout < 4


def _params(forms):
    return [pytest.param(f, s, r, id=f"{f.replace(' ', '_')}-{s[0]}to{s[1]}-{s[4]}x{s[5]}-{r}")
            for f, shapes in forms.items() for i, s in enumerate(shapes) for r in (EC.REGIMES if i == 0 or s in ALL_REGIMES else EC.REGIMES[:1])]


@pytest.fixture(scope="module")
def eng(synth_sd):
    from savsr_amd.engine import HipEngine
    from savsr_amd.archs.savsr_arch import SAVSR
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return HipEngine(synth_sd, SAVSR().cfg, DEV)


@pytest.fixture(scope="module")
def table():
    """Worst ratio per (form, activation, operand subset) over everything the module ran, printed at the end."""
    t = {}
    yield t
    names = [EC.subset_name(s) for s in EC.SUBSETS]
    print("\nworst |got - reference| / bound per form, activation and operand subset (b bias, m mask, 1 res1, 2 res2; max over shapes and regimes):")
    for form in sorted({k[0] for k in t}):
        print(f"  {form:21s}" + " ".join(f"{n:>4s}" for n in names))
        for act in sorted({k[1] for k in t if k[0] == form}):
            print(f"    {act:19s}" + " ".join(f"{t[(form, act, n)]:4.2f}" if (form, act, n) in t else "   ." for n in names))


def _note(table, form, E, r):
    key = (form, EC.act_name(E.act, E.slope), EC.subset_name(E.subset()))
    table[key] = max(table.get(key, 0.0), r)


def _algos(form):
    from savsr_amd import _lib
    return (_lib.CONV_WINOGRAD_Y, _lib.CONV_WINOGRAD_Y_THROUGHPUT) if form == "winograd-y" else (_lib.CONV_DIRECT,)


def _is_wy(algo):
    from savsr_amd import _lib
    return algo in _lib.CONV_WY_FORMS


class _Input:
    """One conv's sources and weight image on the device."""

    def __init__(self, x, wt, wy, f16):
        from savsr_amd import packing as P
        wt = torch.from_numpy(np.ascontiguousarray(wt))
        pack = (P.pack_conv_weight_wy_f16 if wy else P.pack_conv_weight_f16) if f16 else (P.pack_conv_weight_wy if wy else P.pack_conv_weight)
        self.img = pack(wt).to(DEV)
        self.xall = torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32).transpose(1, 2, 0))).to(DEV)       # [h][w][cin]


def _slice_of(t_np, pad_lo, pad_hi):
    """Planar [c][h][w] operand -> (NaN-filled device tensor [h][w][pad_lo + c + pad_hi], channel offset)."""
    c, h, w = t_np.shape
    wide = torch.full((h, w, pad_lo + c + pad_hi), float("nan"))
    wide[..., pad_lo:pad_lo + c] = torch.from_numpy(np.ascontiguousarray(t_np.transpose(1, 2, 0)))
    return wide.to(DEV), pad_lo


class _Conv:
    """One descriptor and everything it points to (kept alive here).  The output is the slice [4, 4 + cout) of a NaN-filled tensor 4
    channels wider (offset 0 where cout % 4 != 0: the kernels then store scalars); res1 / res2 are slices of wider tensors with other
    pitches; E = None is the bare run."""

    def __init__(self, eng, inp, shape, algo, E=None, pool=False, src=None):
        self.eng, self.inp, self.shape, self.algo, self.E, self.with_pool, self.src = eng, inp, shape, algo, E, pool, src
        cin, cout, ks, nsrc, h, w = shape
        q = cout % 4 == 0
        self.ops = {}
        if E is not None:
            if E.bias is not None:
                self.ops["bias"] = torch.from_numpy(E.bias).to(DEV)
            if E.mul is not None:
                self.ops["mul"] = torch.from_numpy(E.mul).to(DEV)
            if E.res1 is not None:
                self.ops["res1"] = _slice_of(E.res1, 4 if q else 1, 4 if q else 1)
            if E.res2 is not None:
                self.ops["res2"] = _slice_of(E.res2, 8 if q else 2, 4 if q else 3)
        self.new_output()

    def new_output(self):
        from savsr_amd import engine as G
        eng, E = self.eng, self.E
        cin, cout, ks, nsrc, h, w = self.shape
        self.off = 4 if cout % 4 == 0 else 0
        self.wide = torch.full((h, w, cout + 4), float("nan"), device=DEV)
        sch = cin // nsrc
        srcs = self.src if self.src is not None else [eng.full(self.inp.xall, sch, i * sch) for i in range(nsrc)]
        kw = {}
        if E is not None:
            kw.update(act=E.act, slope=E.slope, mul_px=self.ops.get("mul"), res2_scale=E.res2_scale if E.res2 is not None else 0.0)
            for k in ("res1", "res2"):
                if k in self.ops:
                    t, o = self.ops[k]
                    kw[k] = G.Src(t, cout, t.shape[-1], o)
        if self.with_pool:
            # the pool's column slice [4, 4 + cout) of rows 8 columns wider, and one spare row: NaN guards on every side
            self.pool = torch.full((eng.pool_rows(h, w) + 1, cout + 8), float("nan"), device=DEV)
            kw["pool"] = (self.pool, 4, cout + 8)
        bias = self.ops.get("bias")
        self.desc = eng.conv_desc("epilogue", srcs, G.Src(self.wide, cout, cout + 4, self.off), h, w,
                                  weights=(self.inp.img, bias, cout, cin, ks, self.algo), **kw)

    def alone(self):
        """The same conv on the same operands with an output of its own."""
        c = copy.copy(self)
        c.new_output()
        return c

    def out_slice(self):
        cout = self.shape[1]
        return self.wide[..., self.off:self.off + cout]

    def result(self) -> np.ndarray:
        cout = self.shape[1]
        guard = torch.cat([self.wide[..., :self.off], self.wide[..., self.off + cout:]], -1)
        assert guard.shape[-1] == 4 and bool(torch.isnan(guard).all())                      # nothing written outside the channel slice
        return np.ascontiguousarray(self.out_slice().detach().cpu().numpy().transpose(2, 0, 1))


def _launch(eng, convs, f16=False):
    """savsr_conv2d_batch(_f16) in launches of savsr_conv2d_max_batch() convs (the engine's own launcher stops at 6)."""
    from savsr_amd import _lib
    fn = eng.lib.savsr_conv2d_batch_f16 if f16 else eng.lib.savsr_conv2d_batch
    nmax = int(eng.lib.savsr_conv2d_max_batch())
    st = torch.cuda.current_stream().cuda_stream
    for i in range(0, len(convs), nmax):
        chunk = [c.desc for c in convs[i:i + nmax]]
        _lib.check(fn((_lib.ConvDesc * len(chunk))(*chunk), len(chunk), st), "savsr_conv2d_batch")


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def _matrix(eng, shape, regime, algo, f16):
    """The 96 descriptors of a (shape, regime, algo): [(conv, its bare conv)], launched; each descriptor has operands of its own.  The
    sigmoid descriptors of the unit regime run on the sigmoid input set (+-0.1 ... +-100 through a selecting weight)."""
    cin, cout, ks, nsrc, h, w = shape
    wy = _is_wy(algo)
    main = _Input(*EC.conv_inputs(cin, cout, ks, h, w, 5, regime), wy, f16)
    sig = _Input(*EC.sigmoid_conv_inputs(cin, cout, ks, h, w, 6), wy, f16) if regime == "unit" else main
    bare = {id(main): _Conv(eng, main, shape, algo)}
    if sig is not main:
        bare[id(sig)] = _Conv(eng, sig, shape, algo)
    convs = []
    for k, (act, slope, sub) in enumerate(EC.matrix()):
        inp = sig if act == EC.SIGMOID else main
        convs.append((_Conv(eng, inp, shape, algo, EC.epilogue(act, slope, sub, EC.operands(cout, h, w, 1000 + k, regime))), bare[id(inp)]))
    for b in bare.values():
        _launch(eng, [b], f16)
    _launch(eng, [c for c, _ in convs], f16)
    return convs


def _check_matrix(eng, table, form, shape, regime, f16):
    algos = _algos(form)
    convs = _matrix(eng, shape, regime, algos[0], f16)
    torch.cuda.synchronize()
    tag = f"{form}{' fp16' if f16 else ''}"
    rows, bad = {}, []
    for c, b in convs:
        a, got = b.result(), c.result()
        assert bool(np.isfinite(a).all()) and bool(np.isfinite(got).all()), c.E.name()
        r = EC.worst_ratio(got, a, c.E)
        act = EC.act_name(c.E.act, c.E.slope)
        rows.setdefault(act, []).append((EC.subset_name(c.E.subset()), r))
        _note(table, tag, c.E, r)
        if not r <= 1.0:
            bad.append((c.E.name(), r))
        if c.E.act == EC.SIGMOID and regime == "unit" and not c.E.subset() and a.size >= 100:
            assert EC.covers_sigmoid_set(a)
            assert bool((got[a < -90] == 0).all()) and bool((got[a > 90] == 1).all())          # expf overflow: exactly 0 / 1
    for act, r in rows.items():
        print(f"{tag} {shape[0]}->{shape[1]} ks{shape[2]} {shape[4]}x{shape[5]} {regime:6s} {act:12s} " + " ".join(f"{s} {v:4.2f}" for s, v in r))
    assert not bad, bad
    if len(algos) > 1:                    # WINOGRAD_Y_THROUGHPUT (strip tiles for the last rows): the same bits
        tp = _matrix(eng, shape, regime, algos[1], f16)
        torch.cuda.synchronize()
        for (c, _), (c2, _) in zip(convs, tp):
            assert _same_bits(c.result(), c2.result()), c.E.name()


@pytest.mark.parametrize("form,shape,regime", _params(FORMS))
def test_every_activation_with_every_operand_subset(eng, table, form, shape, regime):
    """Test 1: NONE, RELU, LRELU 0.2 / 1.5 / -0.25 and SIGMOID, each with all 16 subsets of {bias, mask, res1, res2}, inside the derived
    bound on every output, in four launches of 24 convs with mixed epilogues."""
    _check_matrix(eng, table, form, shape, regime, False)


@pytest.mark.parametrize("form,shape,regime", _params(F16_FORMS))
def test_every_activation_with_every_operand_subset_f16(eng, table, form, shape, regime):
    """Test 4: the same through savsr_conv2d_batch_f16 on fp16 images, the bare run being the fp16 bare run: "the same fp32 epilogue", so the
    same bounds."""
    _check_matrix(eng, table, form, shape, regime, True)


@pytest.mark.parametrize("form,shape,regime,f16", [pytest.param(*p.values, f16, id=p.id + ("-fp16" if f16 else "-fp32"))
                                                   for f16, forms in ((False, FORMS), (True, F16_FORMS)) for p in _params(forms)])
def test_alone_equals_in_the_mixed_batch(eng, form, shape, regime, f16):
    """Test 2: every descriptor of the matrix launched alone gives the bits it gives among 23 convs with other epilogues (the stale-
    descriptor check; in the Winograd-y form a qualifying conv alone runs conv_wy_kernel<true>, in the batch the generic instantiation)."""
    for algo in _algos(form):
        convs = _matrix(eng, shape, regime, algo, f16)
        solo = [c.alone() for c, _ in convs]
        for s in solo:
            _launch(eng, [s], f16)
        torch.cuda.synchronize()
        for (c, _), s in zip(convs, solo):
            assert _same_bits(c.result(), s.result()), (c.E.name(), algo)


def test_direct_16_row_tiles(eng, table):
    """The 16-row tiling of conv_mfma.hip (PXT = 2): DIRECT_THROUGHPUT takes it from 100 tiles, a 64 -> 64 conv at 100 x 320 has 70 -- ONE
    launch of the bare conv and four representative epilogues (350 tiles), each inside its bound."""
    from savsr_amd import _lib
    shape = (64, 64, 3, 1, 100, 320)
    cin, cout, ks, nsrc, h, w = shape
    assert 2 * ((h + 15) // 16) * ((w + 31) // 32) >= 100
    inp = _Input(*EC.conv_inputs(cin, cout, ks, h, w, 5), False, False)
    ops = [EC.operands(cout, h, w, 50 + k) for k in range(4)]
    es = [EC.epilogue(EC.RELU, 0.0, ("bias", "res1"), ops[0]), EC.epilogue(EC.LRELU, 0.2, EC.OPERANDS, ops[1]),
          EC.epilogue(EC.NONE, 0.0, ("mul", "res1", "res2"), ops[2]), EC.epilogue(EC.SIGMOID, 0.0, ("mul",), ops[3])]
    bare = _Conv(eng, inp, shape, _lib.CONV_DIRECT_THROUGHPUT)
    convs = [_Conv(eng, inp, shape, _lib.CONV_DIRECT_THROUGHPUT, E) for E in es]
    _launch(eng, [bare] + convs)
    torch.cuda.synchronize()
    a = bare.result()
    for c in convs:
        r = EC.worst_ratio(c.result(), a, c.E)
        print(f"direct 16-row 64->64 100x320 {c.E.name()}: {r:4.2f}")
        _note(table, "direct 16-row", c.E, r)
        assert r <= 1.0, c.E.name()


@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("tp", [False, True], ids=["winograd_y", "winograd_y_throughput"])
def test_winograd_y_dispatch(eng, tp, f16):
    """Test 3: a launch whose convs ALL qualify for the straight-line epilogue (max-form activation, any of bias and res1: conv_wy_kernel<true>)
    against the same convs in a launch that also holds one mask conv, which forces the generic instantiation: the shared convs give the same
    bits, and their bounds hold."""
    from savsr_amd import _lib
    algo = _lib.CONV_WINOGRAD_Y_THROUGHPUT if tp else _lib.CONV_WINOGRAD_Y
    shape = (64, 64, 3, 1, 17, 34)
    cin, cout, ks, nsrc, h, w = shape
    inp = _Input(*EC.conv_inputs(cin, cout, ks, h, w, 5), True, f16)
    es = [EC.epilogue(act, slope, sub, EC.operands(cout, h, w, 300 + 4 * i + j))
          for i, (act, slope) in enumerate(EC.ACTS[:3]) for j, sub in enumerate(((), ("bias",), ("res1",), ("bias", "res1")))]
    fast = [_Conv(eng, inp, shape, algo, E) for E in es]
    generic = [c.alone() for c in fast] + [_Conv(eng, inp, shape, algo, EC.epilogue(EC.NONE, 0.0, ("mul",), EC.operands(cout, h, w, 399)))]
    bare = _Conv(eng, inp, shape, algo)
    _launch(eng, fast, f16)
    _launch(eng, generic, f16)
    _launch(eng, [bare], f16)
    torch.cuda.synchronize()
    a = bare.result()
    for c, g in zip(fast, generic):
        assert _same_bits(c.result(), g.result()), c.E.name()
        assert EC.worst_ratio(c.result(), a, c.E) <= 1.0, c.E.name()
    assert EC.worst_ratio(generic[-1].result(), a, generic[-1].E) <= 1.0


@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("wy", [False, True], ids=["direct", "winograd_y"])
def test_fused_pool_with_an_epilogue(eng, wy, f16):
    """Test 5: ReLU + bias + res1 and sigmoid + mask with the fused pool, 19 x 40 (a partial last band and segment): the outputs keep their
    bounds, every pool row equals the float64 sum of the STORED outputs of its cell within 255 * 2^-24 sum |out| (any fp32 order of <= 256
    terms), and nothing is written outside the pool's column slice (NaN guard columns on both sides and a spare row behind the last).  The
    ReLU conv runs once more alone -- in the Winograd-y form that is conv_wy_kernel<true> with pool, bias and res1 -- with the same bits."""
    from savsr_amd import _lib
    shape = (64, 64, 3, 1, 19, 40)
    cin, cout, ks, nsrc, h, w = shape
    algo = _lib.CONV_WINOGRAD_Y if wy else _lib.CONV_DIRECT
    inp = _Input(*EC.conv_inputs(cin, cout, ks, h, w, 5), wy, f16)
    es = [EC.epilogue(EC.RELU, 0.0, ("bias", "res1"), EC.operands(cout, h, w, 70)), EC.epilogue(EC.SIGMOID, 0.0, ("mul",), EC.operands(cout, h, w, 71))]
    bare = _Conv(eng, inp, shape, algo)
    convs = [_Conv(eng, inp, shape, algo, E, pool=True) for E in es]
    solo = convs[0].alone()          # ReLU + bias + res1 with no mask conv beside it: in the Winograd-y form the straight-line instantiation
    _launch(eng, [bare] + convs, f16)
    _launch(eng, [solo], f16)
    torch.cuda.synchronize()
    a = bare.result()
    ntx = (w + 31) // 32
    nrows = ntx * ((h + 7) // 8)
    assert _same_bits(solo.result(), convs[0].result())
    assert torch.equal(solo.pool[:nrows, 4:4 + cout], convs[0].pool[:nrows, 4:4 + cout])
    for c in convs + [solo]:
        out = c.result()
        assert EC.worst_ratio(out, a, c.E) <= 1.0, c.E.name()
        assert c.pool.shape == (nrows + 1, cout + 8)
        guards = (c.pool[:, :4], c.pool[:, 4 + cout:], c.pool[nrows:])                     # left, right, the spare row behind the last
        assert all(bool(torch.isnan(g).all()) for g in guards), c.E.name()
        rows = c.pool[:nrows, 4:4 + cout].double().cpu().numpy()
        worst = 0.0
        for band in range((h + 7) // 8):
            for seg in range(ntx):
                cell = out[:, 8 * band:8 * band + 8, 32 * seg:32 * seg + 32].astype(np.float64)
                err, mag = np.abs(rows[band * ntx + seg] - cell.sum((1, 2))), np.abs(cell).sum((1, 2))
                assert bool((err <= 255 * EC.U * mag).all()), (c.E.name(), band, seg)
                worst = max(worst, float((err / mag).max()))
        print(f"pool {'winograd-y' if wy else 'direct'}{' fp16' if f16 else ''}{' alone' if c is solo else ''} {c.E.name()}: worst row error "
              f"{worst / EC.U:.2f} * 2^-24 of its cell's sum |out|")


@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16"])
def test_signed_zeros(eng, f16):
    """Test 6a: ReLU in the max form (v_max_f32(v, v * 0)) may store -0 where a select stores +0; numerically the same (the bounds above).
    Pinned here: a following conv cannot tell them apart -- a bare conv fed the ReLU output as stored gives the bits it gives for the same
    tensor with every zero +0, from the interior path into both forms and from the partial-channel path (64 -> 16, then 16 -> 1)."""
    from savsr_amd import _lib
    from savsr_amd import engine as G
    for first, second, algo2 in (((64, 64, 3, 1, 12, 33), (64, 64, 3, 1, 12, 33), _lib.CONV_DIRECT),
                                 ((64, 64, 3, 1, 12, 33), (64, 64, 3, 1, 12, 33), _lib.CONV_WINOGRAD_Y),
                                 ((64, 16, 3, 1, 10, 12), (16, 1, 3, 1, 10, 12), _lib.CONV_DIRECT)):
        cin, cout, ks, nsrc, h, w = first
        relu = _Conv(eng, _Input(*EC.conv_inputs(cin, cout, ks, h, w, 5), False, f16), first, _lib.CONV_DIRECT, EC.Epilogue(EC.RELU))
        _launch(eng, [relu], f16)
        y = relu.result()
        assert bool((y == 0).mean() > 0.25) and bool((y > 0).mean() > 0.25)
        stored = relu.wide                                                   # [h][w][cout + 4], the slice at 4; -0 wherever the kernel left one
        plus = stored + 0.0                                                  # every zero +0 (IEEE: -0 + +0 = +0)
        minus = torch.where(stored == 0, torch.full_like(stored, -0.0), stored)          # and every zero -0
        assert bool(torch.signbit(minus[..., 4:][minus[..., 4:] == 0]).all()) and not bool(torch.signbit(plus[..., 4:][plus[..., 4:] == 0]).any())
        inp2 = _Input(np.zeros((second[0], 1, 1), np.float32), EC.conv_inputs(*second[:3], h, w, 8)[1], _is_wy(algo2), f16)
        outs = []
        for t in (stored, plus, minus):
            c = _Conv(eng, inp2, second, algo2, src=[G.Src(t, cout, cout + 4, 4)])
            c.keep = t
            _launch(eng, [c], f16)
            outs.append(c)
        torch.cuda.synchronize()
        assert _same_bits(outs[0].result(), outs[1].result()) and _same_bits(outs[0].result(), outs[2].result()), (first, second, algo2)
        assert bool(np.isfinite(outs[0].result()).all()) and bool((outs[0].result() != 0).any())


NONFINITE = [("direct 3x3", (64, 64, 3, 1, 12, 33)), ("direct partial", (64, 16, 3, 1, 10, 20)), ("direct partial", (16, 1, 3, 1, 10, 20)),
             ("winograd-y", (64, 64, 3, 1, 17, 34))]


@pytest.mark.parametrize("form,shape", NONFINITE, ids=[f"{f.replace(' ', '_')}-{s[0]}to{s[1]}" for f, s in NONFINITE])
def test_nonfinite_accumulators(eng, form, shape):
    """Test 6b: fp16 mode, the `edge` plants of tests/range_cases.py and one -inf beside the +inf (+-inf, and NaN where they meet) under each activation, bare and with
    every operand.  What include/savsr_hip.h documents, on every path: NONE / RELU / LRELU keep a non-finite accumulator non-finite --
    RELU(-inf) = -inf and RELU(NaN) = NaN (the max form; the partial-channel path used fmaxf, which gave 0 for both) --, LRELU multiplies
    an infinity by its slope, SIGMOID gives exactly 0 / 1 / NaN.  The class of every output is the class of the float64 chain on the stored
    accumulator, and an output whose accumulator is finite keeps its bound."""
    cin, cout, ks, nsrc, h, w = shape
    algo = _algos(form)[0]
    _, x, wt = next(R.regimes_f16(cin, cout, ks, h, w, 7, only=("edge",)))
    x = x.numpy().copy()
    assert x[2, 2, 11] == 65520.0 and w >= 14
    x[3, 2, 12] = -70000.0          # one more plant, next to the +inf one in another channel: opposite infinities meet, NaN in the direct form too
    inp = _Input(x, wt.numpy(), _is_wy(algo), True)
    bare = _Conv(eng, inp, shape, algo)
    convs = [_Conv(eng, inp, shape, algo, EC.epilogue(act, slope, sub, EC.operands(cout, h, w, 500 + 2 * i + j)))
             for i, (act, slope) in enumerate(EC.ACTS) for j, sub in enumerate(((), EC.OPERANDS))]
    _launch(eng, [bare] + convs, True)
    torch.cuda.synchronize()
    a = bare.result()
    cls = R.nonfinite_class(torch.from_numpy(a))
    counts = [int((cls == k).sum()) for k in (1, 2, 3)]
    print(f"{form} {cin}->{cout} {h}x{w}: accumulators +inf {counts[0]}, -inf {counts[1]}, NaN {counts[2]} of {a.size}")
    assert min(counts) > 0 and int((cls == 0).sum()) > a.size // 2
    fin = np.isfinite(a)
    for c in convs:
        got = c.result()
        ref, b = EC.reference(a, c.E), EC.bound(a, c.E)
        assert torch.equal(R.nonfinite_class(torch.from_numpy(got)), R.nonfinite_class(torch.from_numpy(ref))), c.E.name()
        assert bool((np.abs(got[fin] - ref[fin]) <= b[fin]).all()), c.E.name()
        if c.E.act == EC.RELU and not c.E.subset():
            assert bool((got[a == -np.inf] == -np.inf).all()) and bool(np.isnan(got[np.isnan(a)]).all())
        if c.E.act == EC.SIGMOID and not c.E.subset():
            assert bool((got[a == -np.inf] == 0).all()) and bool((got[a == np.inf] == 1).all())


@pytest.mark.parametrize("wy", [False, True], ids=["direct", "winograd_y"])
def test_sharpness_on_the_kernels_outputs(eng, wy):
    """Test 7: every mutant of tests/epilogue_cases.py (bf16 slope or scale, swapped steps, a neighbour's mask or residual, fmaxf for
    LeakyReLU, an absent operand read as present, ...) used as the REFERENCE for the kernel's own output fails the bound on at least half of
    the elements it can change; the unmutated reference passes on every element."""
    from savsr_amd import _lib
    shape = (64, 64, 3, 1, 12, 33)
    cin, cout, ks, nsrc, h, w = shape
    algo = _lib.CONV_WINOGRAD_Y if wy else _lib.CONV_DIRECT
    inp = _Input(*EC.conv_inputs(cin, cout, ks, h, w, 5), wy, False)
    ops = EC.operands(cout, h, w, 21)
    names = [n for n in EC.MUTANTS if EC.mutant_applies(n, cout)]
    bare = _Conv(eng, inp, shape, algo)
    convs = [_Conv(eng, inp, shape, algo, EC.mutant_epilogue(n, ops)) for n in names]
    _launch(eng, [bare] + convs)
    torch.cuda.synchronize()
    a = bare.result()
    for n, c in zip(names, convs):
        got = c.result()
        assert EC.worst_ratio(got, a, c.E) <= 1.0, n
        cnt, share = EC.mutant_share(n, a, c.E, ops, got)
        print(f"sharpness {'winograd-y' if wy else 'direct'} {n:20s}: fails the bound on {100 * share:5.1f} % of the {cnt} elements it can change")
        assert cnt >= a.size // 4 and share >= 0.5, (n, share)
