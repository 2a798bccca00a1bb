"""The SATU kernels (satu.hip: forms "plain", "p27", "q"; satu_nf.hip: "nf" at num_feat 32) stage by stage against the float64 references of
tests/satu_cases.py, with PER-OUTPUT bounds relative to each output's own magnitude sum S, across weight sets, head sets and data regimes.
The C entry points are called with the test's own buffers (NaN-filled, with guard records / planes); every launch of the tuned HR stage runs
without a tiling (static walk, global gathers) and, under every wave split, with an LDS window and without one (dynamic tile queue): same bits.

LR stage, per record element:   A: |got - exact| <= 2^-13 S_A;  B, C: |got - exact| <= 2^-14 S and |got - emul| <= T_ACC S;  S == 0 => 0.
HR stage, per output:           |got - exact| <= 2^-14 S + 2 DELTA_POS S4, DELTA_POS = 4 * 2^-24 max(h, w);  S == 0 => 0; all taps outside =>
                                fusion_b, bit for bit.
(derivations: the docstring of tests/satu_cases.py)

Measured on an MI355X (this file's own run; worst ratio over the shapes of each test, forms plain / p27 = q / nf):
  LR stage, A: |got - exact| of S_A (* 2^-17; the bound is 16):   gauss 0.03 / 0.04 / 0.06, decades 0.40 / 0.36 / 0.32, mean50 0.03 / 0.03 / 0.05,
        vsmooth 0.03 / 0.03 / 0.06, sparse 1.07 / 0.91 / 1.46, heavy 1.62 / 1.52 / 1.25, hole 0.06 / 0.06 / 0.09, impulse 1.66 / 1.64 / 1.85;
        wdecades 2.85 / 2.68 / 3.06, negk 0.24 / 0.29 / 0.33, addressed 2.35 / 2.83 / 3.50 (the worse of `decades` and `impulse`)
  LR stage, B and C: |got - exact| of S (* 2^-17; the bound is 8): gauss 0.67 / 0.56 / 0.86, decades 1.74 / 1.94 / 2.56, mean50 0.40 / 0.38 / 0.51,
        vsmooth 0.56 / 0.51 / 0.90, sparse 2.88 / 3.37 / 3.21, heavy 2.92 / 2.50 / 2.59, hole 0.89 / 0.83 / 1.24, impulse 2.83 / 3.16 / 2.73;
        wdecades 2.83 / 2.92 / 2.78, negk 2.83 / 3.16 / 2.73, addressed 2.59 / 2.70 / 2.47
  LR stage, B and C: |got - emul| of S (T_ACC = 3.3e-6):           0.8e-7 .. 5.4e-7 in every regime (K = 64: a sixth of T_ACC)
  HR stage (plain / p27 / nf), |got - exact| of the bound 2^-14 S + 2 DELTA_POS S4:  gauss 0.12 / 0.13 / 0.13, decades 0.20 / 0.17 / 0.13,
        mean50 0.09 / 0.10 / 0.10, vsmooth 0.13 / 0.13 / 0.14, sparse 0.22 / 0.22 / 0.14, heavy 0.22 / 0.19 / 0.14; by head set: mlp 0.22,
        zero 0.20, integer 0.20, half 0.19, straddle 0.21, wide 0.22, r_sat 0.22.  Of S alone (* 2^-17, not asserted): 5 .. 10 on gauss / mean50 /
        vsmooth, up to 430 on sparse / heavy under `half` -- the position term: an output whose gathered values nearly cancel in S keeps S4
  the engine's own plans (15 .. 52 per shape, each with and without its window) under `straddle` / `wide`, `decades` record: same bits, 0.08 .. 0.15 of the bound
  probe: worst position error 2.76 * 2^-24 max(h, w) (DELTA_POS = 4 of them); phase table: 0.003 of its derived bound; q form: 0.07 of its bound
  sharpness: lo half of one kernel_conv group zeroed: 5 .. 69 dominated outputs, all outside the bound, 47 100 of 47 520 untouched, all inside;
        one k step of Wb: 1024 / 1024; one k step of wbe: 63 .. 79 dominated, all outside; |got - emulated defect| 1.7 (LR), 1.1 (HR) * 2^-17 S
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import range_cases as R
from tests import satu_cases as SC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
TUNED = ("plain", "p27", "q")
REC = dict(plain=160, p27=96, q=96, nf=80)
PLANES = dict(plain=64, p27=27, nf=27)
WORST = {}


def _note(key, value):
    """The worst value per key over the session, printed as it grows (the module docstring's table is read off these lines)."""
    if value > WORST.get(key, -1.0):
        WORST[key] = value
    return WORST[key]


def _up(d):
    return {k: v.to(DEV).contiguous() for k, v in d.items()}


def _pad4(a):
    a = np.ascontiguousarray(a).reshape(-1)
    pad = (-len(a)) % 4
    return torch.from_numpy(np.concatenate([a, np.repeat(a[-1:], pad)]) if pad else a).to(DEV)


class Rig:
    """The packed SATU operands of one state dict on the device and the launches of both stages through the C ABI.  The structs hold raw
    addresses: the object keeps every tensor alive."""

    def __init__(self, sd, c):
        from savsr_amd import _lib
        from savsr_amd.packing import pack_satu_heads, pack_satu_nf, pack_satu_tuned, struct_of
        assert torch.cuda.is_available(), "gpu tests need an MI355X"
        self.sd, self.c, self.lib, self.check = sd, c, _lib.load(), _lib.check
        self.check(self.lib.savsr_prepare_device(), "savsr_prepare_device")
        self.heads = _up(pack_satu_heads(sd))
        self.t, self.w = {}, {}
        if c == 64:
            self.host = {f: pack_satu_tuned(sd, f) for f in TUNED}
            self.t = {f: _up(self.host[f]) for f in TUNED}
            for f in TUNED:
                self.w[f] = struct_of(_lib.SatuWeights, self.heads, self.t["plain"], self.t[f])
            self.w_heads = self.w["plain"]
        else:
            self.t["nf"] = _up(pack_satu_nf(sd, c))
            self.w["nf"] = struct_of(_lib.SatuNfWeights, self.t["nf"], C=c)
            self.w_heads = struct_of(_lib.SatuWeights, self.heads, self.t["nf"], rename={"wbe": "wbe_w"})
        self.sched = torch.zeros(16, dtype=torch.int32, device=DEV)
        self._axes = {}

    def edited(self, form, **images):
        """The weights of `form` with some images replaced by host tensors edited by the caller."""
        from savsr_amd import _lib
        from savsr_amd.packing import struct_of
        self._edit = _up(images)
        return struct_of(_lib.SatuWeights, self.heads, self.t["plain"], self.t[form], self._edit)

    # ---- LR stage: x, st channel-last device tensors, element (y, x, ch) at base + (y row_px + x) pix + ch
    def lr(self, form, xd, std, pix, row_px, h, w, weights=None):
        """-> the record [h, w, REC] (device); it sat NaN-filled between one NaN guard record in front and one behind, checked intact."""
        rec = REC[form]
        buf = torch.full((h * w + 2, rec), NAN, device=DEV)
        fn = dict(plain=self.lib.savsr_satu_lr_stage, p27=self.lib.savsr_satu_lr_stage_tail, q=self.lib.savsr_satu_lr_stage_tail,
                  nf=self.lib.savsr_satu_nf_lr_stage)[form]
        wts = weights if weights is not None else self.w[form]
        self.check(fn(C.byref(wts), xd.data_ptr(), std.data_ptr(), pix, row_px, h, w, buf[1:].data_ptr(), torch.cuda.current_stream().cuda_stream), form)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all()), "guard records"
        return buf[1:-1].view(h, w, rec)

    def lr_planar(self, form, x, st, **kw):
        c, h, w = x.shape
        self._in = (x.permute(1, 2, 0).contiguous().to(DEV), st.permute(1, 2, 0).contiguous().to(DEV))
        return self.lr(form, *self._in, c, w, h, w, **kw)

    # ---- HR stage
    def axes(self, h, w, sc):
        key = (h, w, tuple(sc))
        if key not in self._axes:
            ax = SC.unique_axes(h, w, sc)
            d = {k: _pad4(ax[k]) for k in ("uh", "uw", "ih", "iw", "gyn", "gxn")}
            n_uh, n_uw = len(ax["uh"]), len(ax["uw"])
            table = torch.full((n_uh * n_uw * 8 + 8,), NAN, device=DEV)
            st = torch.cuda.current_stream().cuda_stream
            self.check(self.lib.savsr_satu_phase_table(C.byref(self.w_heads), d["uh"].data_ptr(), n_uh, d["uw"].data_ptr(), n_uw, 1.0 / sc[1], 1.0 / sc[0],
                                                       table.data_ptr(), st), "phase_table")
            ptab = None
            if n_uh * n_uw > 256:
                ptab = torch.full((ax["H"] * ax["W"] * 8 + 8,), NAN, device=DEV)
                self.check(self.lib.savsr_satu_expand_table(table.data_ptr(), n_uw, d["ih"].data_ptr(), d["iw"].data_ptr(), h, w, ax["H"], ax["W"],
                                                            ptab.data_ptr(), st), "expand_table")
            torch.cuda.synchronize()
            assert bool(torch.isnan(table[-8:]).all()) and (ptab is None or bool(torch.isnan(ptab[-8:]).all()))
            host = table[:-8].view(n_uh, n_uw, 8).cpu().numpy()
            self._axes[key] = dict(ax, dev=d, n_uh=n_uh, n_uw=n_uw, table=table, ptab=ptab, table_host=host, tab=SC.per_pixel_table(host, ax),
                                   ptab_host=None if ptab is None else ptab[:-8].view(ax["H"], ax["W"], 8).cpu().numpy())
        return self._axes[key]

    def plans(self, form, ax, h, w, sc):
        """None (no tiling: static walk, global gathers) and, per wave split, an 8-row (4 where 8 do not fit) x 32 tile with the LDS window the
        table's offset range needs -- the engine's plan (launch._plan_hr_tiling) with one tile shape -- and the same tile without a window."""
        from savsr_amd import _lib
        out = [None]
        if form == "nf":
            return out
        tab = ax["table_host"].reshape(-1, 8)
        ox, oy = np.concatenate([tab[:, 4], tab[:, 6]]), np.concatenate([tab[:, 5], tab[:, 7]])
        nvar = int(self.lib.savsr_satu_hr_variants()) if form != "plain" else 1
        for variant in range(nvar):
            t = _lib.SatuTiling()
            t.variant, t.table_entries, t.step_x, t.step_y = variant, ax["n_uh"] * ax["n_uw"], 1.0 / float(sc[1]), 1.0 / float(sc[0])
            t.tile_rows, t.tile_cols32, t.lr_rows, t.lr_cols, t.off_min_x, t.off_min_y = 8, 1, 0, 0, 0.0, 0.0      # (no window fits: a tiling without one)
            for trows in (8, 4):
                lr_c = min(max(int(np.ceil(32 / sc[1] + float(ox.max() - ox.min()))) + 2, 2), w)
                lr_r = min(int(np.ceil(trows / sc[0] + float(oy.max() - oy.min()))) + 2, h)
                if self.lib.savsr_satu_hr_lds_bytes(int(form != "plain"), ax["n_uh"] * ax["n_uw"], trows, 1, lr_r, lr_c) <= 159 * 1024:
                    t.tile_rows, t.lr_rows, t.lr_cols, t.off_min_x, t.off_min_y = trows, lr_r, lr_c, float(ox.min()), float(oy.min())
                    break
            out.append(t)
            if t.lr_rows:                                      # the same tile under this wave split without its window
                t0 = _lib.SatuTiling.from_buffer_copy(t)
                t0.lr_rows, t0.lr_cols = 0, 0
                out.append(t0)
        return out

    def hr(self, form, rec, h, w, sc, tiling=None, weights=None):
        """-> the planes [64 | 27, H, W] (device).  They sat NaN-filled at a pitch of H W + 20 floats with one spare plane behind: the padding
        and the spare plane are checked intact."""
        ax = self.axes(h, w, sc)
        H, W, n, d = ax["H"], ax["W"], PLANES[form], ax["dev"]
        pitch = H * W + 20
        out = torch.full((n + 1, pitch), NAN, device=DEV)
        wts = weights if weights is not None else self.w[form]
        args = (C.byref(wts), rec.data_ptr(), h, w, ax["table"].data_ptr(), ax["n_uh"], ax["n_uw"], d["ih"].data_ptr(), d["iw"].data_ptr(),
                None if ax["ptab"] is None else ax["ptab"].data_ptr(), d["gyn"].data_ptr(), d["gxn"].data_ptr(), H, W)
        st = torch.cuda.current_stream().cuda_stream
        if form == "nf":
            self.check(self.lib.savsr_satu_nf_hr(*args, out.data_ptr(), pitch, st), "nf_hr")
        else:
            fn = self.lib.savsr_satu_hr_upsample if form == "plain" else self.lib.savsr_satu_hr_tail
            self.check(fn(*args, None if tiling is None else C.byref(tiling), None if tiling is None else self.sched.data_ptr(), out.data_ptr(), pitch, st), form)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[:n, H * W:]).all()) and bool(torch.isnan(out[n]).all()), "nothing is written between or behind the planes"
        assert not bool(self.sched.any()), "the tile queue is left zero"
        return out[:n, :H * W].view(n, H, W)

    def hr_all_plans(self, form, rec, h, w, sc):
        """The planes (host, float64) of the launch without a tiling; every other plan gives the same bits."""
        ax = self.axes(h, w, sc)
        outs = [self.hr(form, rec, h, w, sc, t) for t in self.plans(form, ax, h, w, sc)]
        for o in outs[1:]:
            assert torch.equal(o, outs[0]), "launch plans differ"
        return outs[0].cpu().double().numpy(), len(outs)


_RIGS = {}


def rig(ws, heads="mlp", c=64, h=0, w=0) -> Rig:
    key = (ws, heads, c) + ((h, w) if heads == "outside" else ())
    if key not in _RIGS:
        _RIGS[key] = Rig(SC.with_heads(SC.weights(ws, c), heads, h, w), c)
    return _RIGS[key]


def _c(form):
    return 32 if form == "nf" else 64


# ----------------------------------------------------------------------------- LR stage
def _check_lr(tag, key, got, ref, strict=True):
    """Per record element: the bound against `exact`, T_ACC against `emul` for B and C, S == 0 => 0.  Prints the worst ratios."""
    e1, e2 = np.abs(got - ref["exact"]), np.abs(got - ref["emul"])
    ka, kbc = ref["kind"] == 0, ref["kind"] != 0
    ra, rb = SC.worst(e1[..., ka], ref["S"][..., ka]) / R.U17, SC.worst(e1[..., kbc], ref["S"][..., kbc]) / R.U17
    rt = SC.worst(e2[..., kbc], ref["S"][..., kbc])
    print(f"{tag}: A {ra:6.3f} * 2^-17 S_A, B C {rb:6.3f} * 2^-17 S, B C vs emul {rt:.2e} S   [worst {key}: A {_note(key + ('A',), ra):.3f}, "
          f"B C {_note(key + ('B',), rb):.3f}, emul {_note(key + ('T',), rt):.2e}]")
    ok1, ok2 = e1 <= ref["bound"], (e2 <= R.T_ACC * ref["S"]) | ka
    if strict:
        assert bool(np.isfinite(got).all()), tag
        assert bool(ok1.all()), (tag, "bound vs exact", float((e1 / np.where(ref["bound"] > 0, ref["bound"], 1))[ref["bound"] > 0].max()))
        assert bool(ok2.all()), (tag, "T_ACC vs emul", rt / R.T_ACC)
        assert bool((got[ref["S"] == 0] == 0).all()), (tag, "S == 0")
    return ok1, ok2


LR_CASES = [("synth", SC.LR_REGIMES), ("wdecades", ("decades", "impulse")), ("negk", ("decades", "impulse")), ("addressed", ("decades", "impulse"))]


@pytest.mark.parametrize("h,w", SC.LR_SHAPES)
@pytest.mark.parametrize("form", TUNED + ("nf",))
def test_lr_stage_per_output(form, h, w):
    """Every data regime on the synth weights, `decades` and `impulse` on the other weight sets: 6 x 7 (one partial tile), 9 x 33 (a second
    row tile of 1 row, a second column tile of 1 pixel), 17 x 40, 8 x 31."""
    c = _c(form)
    for ws, regimes in LR_CASES:
        r = rig(ws, c=c)
        for regime in regimes:
            x, st = SC.lr_data(regime, c, h, w)
            got = r.lr_planar(form, x, st).cpu().double().numpy()
            ref = SC.lr_reference(r.sd, c, form, x, st)
            _check_lr(f"LR {form:5s} {ws:9s} {regime:8s} {h}x{w}", (form, ws if ws != "synth" else regime), got, ref)
            if regime == "hole":
                for kind in range(3):
                    assert bool((ref["S"][..., ref["kind"] == kind] == 0).any())


@pytest.mark.parametrize("form", TUNED + ("nf",))
def test_lr_stage_strided_crop(form):
    """x and st as crops of larger tensors (row pitch > w, 64 of 68 -- 32 of 36 -- floats per pixel) in which everything outside the crop is NaN:
    the record is finite and equals the record of the contiguous copy bit for bit."""
    c = _c(form)
    r = rig("synth", c=c)
    for (h, w), (hp, wp, oy, ox) in (((9, 33), (12, 37, 2, 3)), ((6, 7), (7, 9, 1, 1))):
        x, st = SC.lr_data("gauss", c, h, w)
        want = r.lr_planar(form, x, st)
        big = [torch.full((hp, wp, c + 4), NAN, device=DEV) for _ in range(2)]
        for b, t in zip(big, (x, st)):
            b[oy:oy + h, ox:ox + w, 4:] = t.permute(1, 2, 0).to(DEV)
        xd, std = (b[oy:, ox:, 4:] for b in big)
        assert xd.data_ptr() % 16 == 0
        got = r.lr(form, xd, std, c + 4, wp, h, w)
        assert bool(torch.isfinite(got).all()) and torch.equal(got, want), (form, h, w)


# ----------------------------------------------------------------------------- HR stage
def _check_hr(tag, key, got, ref, rows):
    e = np.abs(got - ref["exact"][:rows])
    s, bound = ref["S"][:rows], ref["bound"][:rows]
    rs, rb = SC.worst(e, s) / R.U17, SC.worst(e, bound)
    print(f"{tag}: {rs:6.3f} * 2^-17 S, {rb:5.3f} of the bound   [worst {key}: {_note(key + ('S',), rs):.3f}, {_note(key + ('bound',), rb):.3f}]")
    assert bool(np.isfinite(got).all()), tag
    assert bool((e <= bound).all()), (tag, rb)
    assert bool((got[s == 0] == 0).all()), (tag, "S == 0")


HR_HEADS = ("mlp", "zero", "integer", "half", "straddle", "wide", "r_sat")


@pytest.mark.parametrize("h,w,sc", SC.HR_SHAPES)
@pytest.mark.parametrize("heads", HR_HEADS)
def test_hr_stage_per_output(heads, h, w, sc):
    """The record supplied by the test in every data regime, the reference evaluated with the launch's own phase table (read back);
    9 x 33 at (4, 4), 13 x 18 at (2.5, 3.5) (W % 4 != 0), 7 x 6 at (1.5, 4), 19 x 23 at (3.9, 3.9) (more than 256 table entries: ptab)."""
    for form in ("plain", "p27", "nf"):
        c = _c(form)
        r = rig("synth", heads, c)
        ax = r.axes(h, w, sc)
        assert (ax["ptab"] is not None) == (ax["n_uh"] * ax["n_uw"] > 256) and (ax["ptab"] is not None or (h, w) != (19, 23))
        for regime in SC.HR_REGIMES:
            rec = SC.hr_record(regime, REC[form], h, w)
            recd = rec.to(DEV)
            got, nplans = r.hr_all_plans(form, recd, h, w, sc)
            assert nplans >= (1 if form == "nf" else 2)
            ref = SC.hr_reference(r.sd, c, form, rec, ax["tab"], ax)
            _check_hr(f"HR {form:5s} {heads:8s} {regime:8s} {h}x{w} x{sc} ({nplans} plans)", (form, heads, regime), got, ref, PLANES[form])


@pytest.mark.parametrize("h,w,sc", SC.HR_SHAPES)
def test_hr_exact_cases(h, w, sc):
    """`outside` heads (offsets of +-(size + 3): all eight taps outside, the +-2 clamp): every output is its fusion_b entry bit for bit, whatever
    the record holds.  An all-zero record with a zero bias (`probe` weights): zero bit for bit."""
    for form in ("plain", "p27", "nf"):
        c = _c(form)
        r = rig("synth", "outside", c, h, w)
        ax = r.axes(h, w, sc)
        for which in range(2):
            assert float(SC.taps32(ax["tab"], ax, h, w, which)["wgt"].max()) == 0.0
        got, _ = r.hr_all_plans(form, SC.hr_record("decades", REC[form], h, w).to(DEV), h, w, sc)
        fb = SC.folded(r.sd, c, form)["fb"][:PLANES[form]]
        assert bool(np.abs(fb).max() > 0) and bool((got == fb[:, None, None]).all()), form
        r = rig("probe", "mlp", c)
        got, _ = r.hr_all_plans(form, torch.zeros(h, w, REC[form], device=DEV), h, w, sc)
        assert bool((got == 0).all()), form


@pytest.mark.parametrize("h,w,sc", SC.HR_SHAPES)
@pytest.mark.parametrize("heads", SC.HEAD_SETS)
def test_probe(heads, h, w, sc):
    """`probe` weights (Wa = 0, Wb = I, b = 0, weight_expand = 0) on `ramp` data, plain form, both stages: the record's B part is x bit for
    bit and output plane c is G(x_c, off) itself -- plane 0 / 1 the sampling position where all four taps are inside, plane 2 the sum of the
    valid tap weights (1 inside, the partial coverage in the straddle band, exactly 0 outside), plane 3 the gathered checkerboard (a tap
    shifted by one flips its sign)."""
    r = rig("probe", heads, 64, h, w)
    x, st = SC.ramp(64, h, w)
    rec = r.lr_planar("plain", x, st)
    ref_lr = SC.lr_reference(r.sd, 64, "plain", x, st)
    kb = torch.from_numpy(ref_lr["kind"] == 1).to(DEV)
    assert torch.equal(rec[..., kb], torch.from_numpy(ref_lr["exact"][..., ref_lr["kind"] == 1]).float().to(DEV))
    assert bool((rec[..., torch.from_numpy(ref_lr["kind"] == 0).to(DEV)] == 0).all())
    got, _ = r.hr_all_plans("plain", rec.contiguous(), h, w, sc)
    ax = r.axes(h, w, sc)
    d = SC.delta_pos(h, w)
    ix, iy = SC.positions64(ax["tab"], ax, h, w, 0)
    t = SC._taps64(ix, iy, h, w)
    inside = (ix >= d) & (ix <= w - 1 - d) & (iy >= d) & (iy <= h - 1 - d)          # all four taps inside, in fp32 as in float64
    ex, ey = np.abs(got[0] - ix)[inside], np.abs(got[1] - iy)[inside]
    if inside.any():
        unit = SC.U24 * max(h, w)
        print(f"probe {heads:8s} {h}x{w} x{sc}: worst position error x {ex.max() / unit:.3f}, y {ey.max() / unit:.3f} * 2^-24 max(h, w) "
              f"(DELTA_POS = 4)   [worst: {_note(('probe',), max(ex.max(), ey.max()) / unit):.3f}]")
        assert float(ex.max()) <= d + 2.0 ** -22 * w and float(ey.max()) <= d + 2.0 ** -22 * h
    cover = t["wgt"].sum(0)
    tol = 8 * d + 2.0 ** -22                       # the HR bound's 2 DELTA_POS S4 with four taps of magnitude 1, plus the fp32 sum
    assert float(np.abs(got[2] - cover).max()) <= tol
    far = (ix <= -1 - d) | (ix >= w + d) | (iy <= -1 - d) | (iy >= h + d)
    assert bool((got[:, far] == 0).all())
    if heads == "outside":
        assert bool(far.all())
    assert bool((np.abs(got[2][inside] - 1.0) <= tol).all())
    chk = SC._gather(x[3:4].double().numpy(), t)[0]
    assert float(np.abs(got[3] - chk).max()) <= tol
    assert bool((got[4:] == 0).all())
    if heads == "straddle":
        assert bool(((cover > 1e-3) & (cover < 1 - 1e-3)).any())


@pytest.mark.parametrize("heads", ["straddle", "wide"])
def test_engine_plans_bit_identical(heads):
    """The engine's own launch plans (launch._plan_hr_tiling: every wave split x every tile shape whose window fits) on a `decades` record
    under `straddle` and `wide` heads: every entry of ax["tail_plans"], with its window and with lr_rows = lr_cols = 0, gives the same bits,
    and they meet the HR bound."""
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.engine import HipEngine
    sd = SC.with_heads(SC.weights("synth"), heads)
    eng = HipEngine(sd, SAVSR().cfg, DEV)
    for h, w, sc in SC.HR_SHAPES[:2]:
        rec = SC.hr_record("decades", 96, h, w)
        recd = rec.to(DEV)
        ax = eng.satu_axes(h, w, sc)
        H, W = ax["H"], ax["W"]
        outs = []
        for til in ax["tail_plans"]:
            keep = (til.lr_rows, til.lr_cols)
            for window in (True, False):
                ax["tiling_tail"] = til
                if not window:
                    til.lr_rows, til.lr_cols = 0, 0
                p27 = torch.full((28, H * W + 20), NAN, device=DEV)
                eng.satu_hr(recd, h, w, sc, p27, H * W + 20, tail_form=True)
                torch.cuda.synchronize()
                til.lr_rows, til.lr_cols = keep
                assert bool(torch.isnan(p27[:27, H * W:]).all()) and bool(torch.isnan(p27[27]).all())
                outs.append(p27[:27, :H * W].clone())
        ax["tiling_tail"] = None
        assert len({(t.variant, t.tile_rows, t.tile_cols32) for t in ax["tail_plans"]}) >= 2
        for o in outs[1:]:
            assert torch.equal(o, outs[0])
        host = ax["table"].view(ax["n_uh"], ax["n_uw"], 8).cpu().numpy()
        axes = SC.unique_axes(h, w, sc)
        ref = SC.hr_reference(sd, 64, "p27", rec, SC.per_pixel_table(host, axes), axes)
        _check_hr(f"HR engine plans {heads} decades {h}x{w} x{sc} ({len(outs)} launches)", ("p27", heads, "decades"),
                  outs[0].view(27, H, W).cpu().double().numpy(), ref, 27)


@pytest.mark.parametrize("regime", ["decades", "sparse"])
def test_row_summed_form(regime):
    """The q form: savsr_satu_hr_tail_q + savsr_tail_gather_q on a supplied record against the float64 tail conv of the float64 P (rows by
    row_q), within the HR bound summed over the nine taps plus the fp32 sum of ten terms (10 * 2^-24 of their magnitude sum)."""
    from savsr_amd.packing import row_q
    for h, w, sc in SC.HR_SHAPES[:2]:
        r = rig("synth", "wide", 64)
        ax = r.axes(h, w, sc)
        H, W, d = ax["H"], ax["W"], ax["dev"]
        rec = SC.hr_record(regime, 96, h, w)
        recd = rec.to(DEV)
        ref = SC.hr_reference(r.sd, 64, "q", rec, ax["tab"], ax)
        tail_b = r.sd["tail.bias"].to(DEV).float().contiguous()
        center = torch.zeros(3, h, w, device=DEV)
        plane, nseam = H * W + 12, ((H * ((W + 31) // 32) * 18 + 63) // 64) * 64
        outs = []
        for til in r.plans("q", ax, h, w, sc)[1:]:
            q9 = torch.full((10, plane), NAN, device=DEV)
            seam = torch.full((nseam + 64,), NAN, device=DEV)
            out = torch.full((4, H, W), NAN, device=DEV)
            st = torch.cuda.current_stream().cuda_stream
            r.check(r.lib.savsr_satu_hr_tail_q(C.byref(r.w["q"]), recd.data_ptr(), h, w, ax["table"].data_ptr(), ax["n_uh"], ax["n_uw"], d["ih"].data_ptr(),
                                               d["iw"].data_ptr(), None if ax["ptab"] is None else ax["ptab"].data_ptr(), d["gyn"].data_ptr(), d["gxn"].data_ptr(),
                                               H, W, C.byref(til), r.sched.data_ptr(), q9.data_ptr(), plane, seam.data_ptr(), nseam, st), "hr_tail_q")
            r.check(r.lib.savsr_tail_gather_q(q9.data_ptr(), plane, seam.data_ptr(), nseam, tail_b.data_ptr(), center.data_ptr(), h, w, H, W,
                                              out.data_ptr(), st), "tail_gather_q")
            torch.cuda.synchronize()
            assert bool(torch.isnan(q9[9]).all()) and bool(torch.isnan(q9[:9, H * W:]).all()) and bool(torch.isnan(seam[nseam:]).all()) and bool(torch.isnan(out[3]).all())
            outs.append(out[:3])
        assert len(outs) >= 1
        for o in outs[1:]:
            assert torch.equal(o, outs[0])
        got = outs[0].cpu().double().numpy()
        pad = lambda a: np.pad(a, ((0, 0), (1, 1), (1, 1)))      # noqa: E731
        pe, pb, ps = pad(ref["exact"]), pad(ref["bound"]), pad(ref["S"])
        exact = np.tile(r.sd["tail.bias"].double().numpy()[:, None, None], (1, H, W))
        bound, mag = np.zeros((3, H, W)), np.abs(exact)
        for ky in range(3):
            for kx in range(3):
                for o in range(3):
                    p = row_q(ky, kx, o)
                    exact[o] += pe[p, ky:ky + H, kx:kx + W]
                    bound[o] += pb[p, ky:ky + H, kx:kx + W]
                    mag[o] += ps[p, ky:ky + H, kx:kx + W]
        bound += 10 * SC.U24 * mag
        e = np.abs(got - exact)
        print(f"q form {regime} {h}x{w} x{sc}: {SC.worst(e, mag) / R.U17:.3f} * 2^-17 of the nine taps' S, {SC.worst(e, bound):.3f} of the bound "
              f"[worst: {_note(('q', regime), SC.worst(e, bound)):.3f}]")
        assert bool(np.isfinite(got).all()) and bool((e <= bound).all())


# ----------------------------------------------------------------------------- phase table
def _table64(sd, ax, sc):
    """The coordinate MLP in float64 on the fp32 (1 / scale, uniq_ch, uniq_cw), and the bound of its fp32 evaluation per entry: a dot product of n
    terms plus its bias errs by <= (n + 1) u of its magnitude sum (any order); ReLU is 1-Lipschitz; the sigmoid has slope <= 1/4 and its own
    arithmetic 1 / (1 + expf(-v)) -- expf within 1 ulp (2 u), a correctly rounded add and divide -- errs by <= r (1 - r) 2 u + 2 u <= 3 u."""
    g = lambda k: sd["upsample." + k].double().numpy()      # noqa: E731
    w0, b0, w2, b2 = g("body.0.weight").reshape(64, 4), g("body.0.bias"), g("body.2.weight").reshape(64, 64), g("body.2.bias")
    wh = np.concatenate([g("routing.0.weight").reshape(4, 64), g("offset.weight").reshape(2, 64), g("st_offset.weight").reshape(2, 64)])
    bh = np.concatenate([g("routing.0.bias"), g("offset.bias"), g("st_offset.bias")])
    n_uh, n_uw = len(ax["uh"]), len(ax["uw"])
    inp = np.stack([np.full((n_uh, n_uw), float(np.float32(1.0 / sc[1]))), np.full((n_uh, n_uw), float(np.float32(1.0 / sc[0]))),
                    np.broadcast_to(ax["uh"].astype(np.float64)[:, None], (n_uh, n_uw)), np.broadcast_to(ax["uw"].astype(np.float64)[None, :], (n_uh, n_uw))], -1)
    u = SC.U24
    a1 = inp @ w0.T + b0
    e1 = 5 * u * (np.abs(inp) @ np.abs(w0).T + np.abs(b0))
    h1 = np.maximum(a1, 0)
    a2 = h1 @ w2.T + b2
    e2 = 65 * u * (h1 @ np.abs(w2).T + np.abs(b2)) + e1 @ np.abs(w2).T
    h2 = np.maximum(a2, 0)
    a3 = h2 @ wh.T + bh
    e3 = 65 * u * (h2 @ np.abs(wh).T + np.abs(bh)) + e2 @ np.abs(wh).T
    out, err = a3.copy(), e3.copy()
    out[..., :4] = 1 / (1 + np.exp(-a3[..., :4]))
    err[..., :4] = e3[..., :4] / 4 + 3 * u
    return out, err


@pytest.mark.parametrize("h,w,sc", SC.HR_SHAPES + ((9, 10, (4, 1.4)),))
def test_phase_table(h, w, sc):
    """Every table entry against the float64 coordinate MLP within the derived fp32 bound; ptab = table[ih][iw] with the offsets normalised
    as (off * 2) / (size - 1) in fp32, bit for bit."""
    worst = 0.0
    for heads in ("mlp", "wide", "r_sat"):
        r = rig("synth", heads, 64)
        ax = r.axes(h, w, sc)
        ref, err = _table64(r.sd, ax, sc)
        e = np.abs(ax["table_host"].astype(np.float64) - ref)
        worst = max(worst, float((e / err).max()))
        assert bool((e <= err).all()), (heads, float((e / err).max()))
        f = np.float32
        want = ax["tab"].copy()
        want[..., 4], want[..., 6] = (want[..., 4] * f(2)) / f(w - 1), (want[..., 6] * f(2)) / f(w - 1)
        want[..., 5], want[..., 7] = (want[..., 5] * f(2)) / f(h - 1), (want[..., 7] * f(2)) / f(h - 1)
        if ax["ptab"] is None:          # (small tables are expanded by the HR stage itself: run the expansion here)
            ptab = torch.full((ax["H"] * ax["W"] * 8 + 8,), NAN, device=DEV)
            d = ax["dev"]
            r.check(r.lib.savsr_satu_expand_table(ax["table"].data_ptr(), ax["n_uw"], d["ih"].data_ptr(), d["iw"].data_ptr(), h, w, ax["H"], ax["W"],
                                                  ptab.data_ptr(), torch.cuda.current_stream().cuda_stream), "expand_table")
            torch.cuda.synchronize()
            assert bool(torch.isnan(ptab[-8:]).all())
            got = ptab[:-8].view(ax["H"], ax["W"], 8).cpu().numpy()
        else:
            got = ax["ptab_host"]
        assert np.array_equal(got, want), heads
    print(f"phase table {h}x{w} x{sc}: worst entry error {worst:.3f} of its derived bound [worst: {_note(('table',), worst):.3f}]")


# ----------------------------------------------------------------------------- sharpness on the device
def _lo_zeroed(img, groups):
    img = img.clone().view(-1, 2, 512)
    for gidx in groups:
        assert bool((img[gidx, 1] != 0).any())
        img[gidx, 1] = 0
    return img.reshape(-1)


def _sharp(tag, got, ref, explain, ratio=1e3):
    """The bound fails in every output the slot dominates (at least 3) and holds in every output the slot does not touch (S_slot <= 2^-7 S: a
    lost lo half moves those by <= 2^-15 S); the emulation of the same defect explains the output within `explain` S."""
    viol = np.abs(got - ref["exact"]) > ref["bound"]
    dom = (ref["S_slot"] >= ratio * (ref["S"] - ref["S_slot"])) & (ref["S"] > 0)
    untouched = ref["S_slot"] <= 2.0 ** -7 * ref["S"]
    rx = SC.worst(np.abs(got - ref["emul"]), ref["S"])
    print(f"{tag}: dominated {int(dom.sum())}, violating {int(viol.sum())}, untouched {int(untouched.sum())} of {viol.size}; "
          f"|got - emulated defect| {rx / R.U17:.3f} * 2^-17 S")
    assert int(dom.sum()) >= 3 and bool(viol[dom].all()), tag
    assert not bool(viol[untouched].any()), tag
    assert rx <= explain, tag


@pytest.mark.parametrize("drop", [("kconv", 7, 1, 2), ("kconv", 24, 0, 0), ("wb", 1)])
def test_sharpness_lr_lo_half_of_one_slot_zeroed(drop):
    """`addressed` x `impulse`, plain form: the lo half of one (tap, cg, ks) group of kconv_w / of one k step of proj_w's Wb tiles zeroed in
    the packed image on the host, handed to the unmodified kernel."""
    from savsr_amd.packing import group_kconv, group_proj_tuned
    r = rig("addressed")
    h, w = 9, 33
    x, st = SC.lr_data("impulse", 64, h, w)
    if drop[0] == "kconv":
        wts = r.edited("plain", kconv_w=_lo_zeroed(r.host["plain"]["kconv_w"], [group_kconv(*drop[1:], 64)]))
    else:
        wts = r.edited("plain", proj_w=_lo_zeroed(r.host["plain"]["proj_w"], [group_proj_tuned(1, t, drop[1], 2) for t in range(2)]))
    got = r.lr_planar("plain", x, st, weights=wts).cpu().double().numpy()
    _sharp(f"sharpness LR {drop}", got, SC.lr_reference(r.sd, 64, "plain", x, st, drop=drop), SC.BOUND_A)
    clean = r.lr_planar("plain", x, st).cpu().double().numpy()
    _check_lr("sharpness LR, unedited image", ("plain", "addressed"), clean, SC.lr_reference(r.sd, 64, "plain", x, st))


@pytest.mark.parametrize("ks", [0, 1])
def test_sharpness_hr_lo_half_of_one_k_step_zeroed(ks):
    """`addressed` weights, a record whose (A, B) floats are 1e-4 of its C-stack, plain form: the lo half of k step ks of wbe_w zeroed.
    (Dominance >= 10^2: a row of Wb E has 16 entries of ~1e-4 in the other k step beside its one O(1) entry; at a share of 0.99 the lost lo
    half, >= 2^-10 of the term by construction, is still 15 x the bound.)"""
    from savsr_amd.packing import group_wbe
    r = rig("addressed")
    h, w, sc = 7, 6, (1.5, 4)
    rec = SC.hr_record("gauss", 160, h, w).clone()
    rec[..., :128] *= 1e-4
    ax = r.axes(h, w, sc)
    wts = r.edited("plain", wbe_w=_lo_zeroed(r.host["plain"]["wbe_w"], [group_wbe(t, ks) for t in range(2)]))
    got = r.hr("plain", rec.to(DEV), h, w, sc, weights=wts).cpu().double().numpy()
    _sharp(f"sharpness HR wbe k step {ks}", got, SC.hr_reference(r.sd, 64, "plain", rec, ax["tab"], ax, defect=("wbe", ks)), SC.BOUND_B, ratio=1e2)
    clean, _ = r.hr_all_plans("plain", rec.to(DEV), h, w, sc)
    _check_hr("sharpness HR, unedited image", ("plain", "addressed", "gauss"), clean, SC.hr_reference(r.sd, 64, "plain", rec, ax["tab"], ax), 64)
