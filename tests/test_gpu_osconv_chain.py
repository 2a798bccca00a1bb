"""The fp32 side kernels of osconv.hip through the C ABI against the float64 references of tests/osconv_cases.py: the OSConv weight chain stage
by stage (partial -> v1 -> v2 -> att -> weight image in the direct and the Winograd-y order), each stage evaluated in float64 on what the launch
itself wrote for the stage before, with PER-ELEMENT bounds relative to the element's own magnitude sum; the fused path against the unfused one,
batches against solo launches, the refusals; the RCAN SE gate with its scale-residual pass; the pooled channel sums.  Every output sits in a
NaN-filled buffer of the test's own with a guard region behind it.  (derivations: the docstring of tests/osconv_cases.py)

Measured on an MI355X (this file's own run; worst |got - exact| as a fraction of the element's derived bound, network geometries / edge
geometries; every bound held at the first run, none was adjusted):
  v1 of the partials:       gauss 0.054 / 0.153, mean50 0.114 / 0.105, altsign 0.038 / 0.107, integers 0.022 / 0.036, zero 0.203 / 0.203,
                            lastblock 0.281 / 0.310, decades 0.053 / 0.063; the pooled mean alone (`probe`): mean50 0.154 / 0.149, integers 0.029 (bit for bit)
  v2 of the launch's v1:    gauss 0.292 / 0.197, mean50 0.163 / 0.183, altsign 0.205 / 0.283, integers 0.132 / 0.186, zero 0.172 / 0.217,
                            lastblock 0.252 / 0.291, decades 0.174 / 0.281
  sigmoid gates of its v2:  synth 0.180 / 0.272, probe 0.179 / 0.282, dead 0.150 / 0.265, sat 0.029 / 0.088, uniform_k 0.176 / 0.265, decades 0.183 / 0.275
  softmax of its v2:        synth 0.070 / 0.092, probe 0.050 / 0.096, dead 0.042 / 0.079, sat 0.029 / 0.037, uniform_k 0 / 0.031 (fl(1 / K) bit for bit),
                            decades 0.059 / 0.085
  direct image of its att:  synth 0.483 / 0.491, sat 0.479 / 0.480, uniform_k 0.386 / 0.488, decades 0.475 / 0.490
  Winograd-y image:         synth 0.486 / 0.478, sat 0.481 / 0.482, uniform_k 0.347 / 0.427, decades 0.475 / 0.472
        (the images sit at half their bound wherever the split term 2^-16 |exact| leads it: hi + lo misses x by up to 2^-17 |x| in practice)
  fp16 images:              0.500 ulp at every geometry, both orders, synth and uniform_k banks (the criterion is 1)
  sharpness:                bank 0's (chunk 1, tap 5) group rounded to bf16: 465 dominated entries, all outside the bound (480 outside in all), 36 352
                            untouched, all inside; bank 7 zeroed for 32 output channels: 18 432 of 18 432 outside, 18 432 untouched inside
  SE gate, (c, cmid):       (64, 4) 0.204, (32, 2) 0.263, (16, 1) 0.236, (4, 1) 0.210, (128, 8) 0.131, (64, 9) 0.132, (128, 20) 0.050 -- the worst regime
                            is `lastblock` or `zero` (the sigmoid's own 3 u leads the bound), mean50 (saturated gates) <= 0.010
  channel sums, src_ch:     16: 0.025, 32: 0.032, 64: 0.059 of gamma(ceil(per / PL) + PL) S; integer data bit for bit
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import osconv_cases as OC
from tests.range_cases import T_ACC, U17      # noqa: F401  (the units the SATU / conv files quote; the bounds here are osconv_cases')
from tests.satu_cases import U24

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
F32 = np.float32
GUARD = 64
WORST = {}
IMAGE_SETS = ("synth", "sat", "uniform_k", "decades")


def _note(key, value):
    """The worst value per key over the session, printed as it grows (the module docstring's table is read off these lines)."""
    if value > WORST.get(key, -1.0):
        WORST[key] = value
    return WORST[key]


def _klass(geom):
    return "network" if geom in OC.NETWORK_GEOMS else "edge"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nan(n):
    return torch.full((n + GUARD,), NAN, device=DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Rig:
    """One weight set at one geometry on the device and the launches of the weight chain through the C ABI.  The descriptors hold raw
    addresses: the object keeps every tensor alive."""
    KEYS = ("l1_w", "l1_b", "l2_w", "l2_b", "fc_w", "bn_scale", "bn_shift", "ch_w", "ch_b", "fl_w", "fl_b", "sp_w", "sp_b", "kn_w", "kn_b")

    def __init__(self, w, geom):
        from savsr_amd import _lib
        from savsr_amd.packing import conv_pack_index, conv_wy_pack_index
        assert torch.cuda.is_available(), "gpu tests need an MI355X"
        self.w, self.geom, self.lib, self._lib = w, geom, _lib.load(), _lib
        _lib.check(self.lib.savsr_prepare_device(), "savsr_prepare_device")
        cin, cout, hidden, knum = geom
        self.idx, self.elems = conv_pack_index(cout, cin, 3)
        assert self.elems == self.lib.savsr_conv_packed_elems(cout, cin, 3)
        g = np.random.RandomState(cin + cout)
        for co, ci, tap in [(0, 0, 0), (cout - 1, cin - 1, 8)] + [(int(g.randint(cout)), int(g.randint(cin)), int(g.randint(9))) for _ in range(32)]:
            assert self.idx.reshape(cout, cin, 9)[co, ci, tap] == self.lib.savsr_conv_pack_index(cout, cin, 3, co, ci, tap)
        self.idx_wy = None
        if cout % 64 == 0:
            self.idx_wy, self.elems_wy = conv_wy_pack_index(cout, cin)
            assert self.elems_wy == self.lib.savsr_conv_wy_packed_elems(cout, cin) == self.elems * 4 // 3
            for pos, co, ci, kx in [(3, cout - 1, cin - 1, 2)] + [(int(g.randint(4)), int(g.randint(cout)), int(g.randint(cin)), int(g.randint(3))) for _ in range(32)]:
                assert self.idx_wy.reshape(4, cout, cin, 3)[pos, co, ci, kx] == self.lib.savsr_conv_wy_pack_index(cout, cin, co, ci, pos, kx)
        self.t = {k: _dev(w[k]) for k in self.KEYS}
        self.bank = self.pack_bank(w["bank"])
        self._keep = []

    def pack_bank(self, bank):
        """[knum][cout][cin][3][3] fp32 -> [knum][elems] on the device: W at its pack index, zeros elsewhere."""
        knum = bank.shape[0]
        out = np.zeros((knum, self.elems), dtype=F32)
        out[:, self.idx] = bank.reshape(knum, -1)
        return _dev(out)

    def out_bufs(self, wy=False, f16=False):
        cin, cout, hidden, knum = self.geom
        n = (self.elems_wy if wy else self.elems) // (2 if f16 else 1)          # floats: two bf16 parts, or one fp16 part
        return dict(v1=_nan(2 * cin), v2=_nan(cin), att=_nan(OC.ngate(self.geom)), img=_nan(n))

    def desc(self, partial, sc, inv_n, bufs, wy=False, fused=False, bank=None):
        cin, cout, hidden, knum = self.geom
        d = self._lib.OSConvAttnDesc()
        d.cin, d.cout, d.hidden, d.knum = cin, cout, hidden, knum
        d.inv_sh, d.inv_sw = (float(v) for v in OC.inv_scales(sc))
        d.partial, d.nblk, d.inv_n = partial.data_ptr(), partial.shape[0], float(inv_n)
        for k in self.KEYS:
            setattr(d, k, self.t[k].data_ptr())
        d.v1, d.v2, d.att, d.wimg_out = (bufs[k].data_ptr() for k in ("v1", "v2", "att", "img"))
        d.bank, d.nunits = (self.bank if bank is None else bank).data_ptr(), self.elems // 8
        d.wy, d.fused = int(wy), int(fused)
        self._keep = [partial, bufs, bank]
        return d

    def launch(self, descs, f16=False):
        fn = self.lib.savsr_osconv_weights_batch_f16 if f16 else self.lib.savsr_osconv_weights_batch
        arr = (self._lib.OSConvAttnDesc * len(descs))(*descs)
        rc = fn(arr, len(descs), _stream())
        torch.cuda.synchronize()
        return rc

    def run(self, partial, sc, inv_n, wy=False, fused=False, f16=False, bank=None):
        """One solo launch -> its buffers (device, guards checked) and host copies of v1, v2, att (fp32 numpy)."""
        pd = _dev(partial)
        bufs = self.out_bufs(wy, f16)
        self._lib.check(self.launch([self.desc(pd, sc, inv_n, bufs, wy, fused, bank)], f16), "savsr_osconv_weights_batch")
        return self.finish(bufs, fused)

    def finish(self, bufs, fused):
        cin = self.geom[0]
        for k, v in bufs.items():
            assert bool(torch.isnan(v[-GUARD:]).all()), ("guard region behind", k)
        if fused:
            assert bool(torch.isnan(bufs["v1"]).all()), "the fused path leaves v1 alone"
        out = dict(bufs)
        for k, n in (("v1", 2 * cin), ("v2", cin), ("att", OC.ngate(self.geom))):
            out[k + "_h"] = bufs[k][:n].cpu().numpy()
        return out

    def decode(self, img, wy=False, f16=False):
        """The image's entries in the order of (wy_)pack_index as float64 -- [cout][cin][3][3] or [4][cout][cin][3] -- after checking that every
        entry the index does not address is zero (in both halves)."""
        cin, cout, hidden, knum = self.geom
        idx, total = (self.idx_wy, self.elems_wy) if wy else (self.idx, self.elems)
        mask = np.ones(total, dtype=bool)
        mask[idx] = False
        if f16:
            part = img[:total // 2].view(torch.float16).double().cpu().numpy()
            assert bool((part[mask] == 0).all()), "unaddressed entries"
        else:
            halves = img[:total].view(torch.bfloat16).view(-1, 2, 512).double().cpu().numpy()
            hi, lo = halves[:, 0].reshape(-1), halves[:, 1].reshape(-1)
            assert bool((hi[mask] == 0).all()) and bool((lo[mask] == 0).all()), "unaddressed entries"
            part = hi + lo
        return part[idx].reshape((4, cout, cin, 3) if wy else (cout, cin, 3, 3))


_RIGS = {}


def rig(ws, geom) -> Rig:
    if (ws, geom) not in _RIGS:
        _RIGS[(ws, geom)] = Rig(OC.weights(ws, geom), geom)
    return _RIGS[(ws, geom)]


def _check(tag, key, got, ref, zero_S=True):
    """Per element: finite, inside the bound, S == 0 => 0.  Prints the worst ratio of the bound."""
    got = got.astype(np.float64)
    e = np.abs(got - ref["exact"])
    r = OC.worst(e, ref["bound"])
    _note(key, r)
    assert bool(np.isfinite(got).all()), tag
    assert bool((e <= ref["bound"]).all()), (tag, r)
    if zero_S:
        s = ref["T"] if "T" in ref else ref["S"]
        assert bool((got[s == 0] == 0).all()), (tag, "S == 0")
    return r


def _bits(t):
    return t.view(torch.int32)


# ----------------------------------------------------------------------------- 1. the stages, unfused
@pytest.mark.parametrize("geom", OC.GEOMS)
def test_stages_per_element(geom):
    """Every weight set x every partial regime x every nblk (the two scale pairs alternating), three launches (l1, l2, aggregate): v1 against
    float64 of the partials, v2 of the launch's v1, att of the launch's v2; the image (direct, and Winograd-y where cout % 64 == 0) of the
    launch's att, on `gauss` and `decades` partials under the weight sets that bear on it.  And what the weight sets promise, exactly."""
    cin, cout, hidden, knum = geom
    kl = _klass(geom)
    for ws in OC.WEIGHT_SETS:
        r = rig(ws, geom)
        w = r.w
        for i, regime in enumerate(OC.REGIMES):
            for j, nblk in enumerate(OC.NBLKS):
                sc = OC.SCALES[(i + j) % 2]
                p, inv_n = OC.partials(regime, nblk, cin), OC.inv_n_of(nblk)
                ish, isw = OC.inv_scales(sc)
                tag = f"{geom} {ws} {regime} nblk {nblk} x{sc}"
                out = r.run(p, sc, inv_n)
                l1 = OC.l1_reference(w, p, ish, isw, inv_n)
                _check(tag + " v1", ("v1", kl, regime), out["v1_h"], l1)
                _check(tag + " v2", ("v2", kl, regime), out["v2_h"], OC.l2_reference(w, out["v1_h"]))
                att = OC.att_reference(w, out["v2_h"])
                ns = att["sig"]
                _check(tag + " gates", ("gates", kl, ws), out["att_h"][:ns], dict(exact=att["exact"][:ns], bound=att["bound"][:ns]), zero_S=False)
                _check(tag + " ka", ("ka", kl, ws), out["att_h"][ns:], dict(exact=att["exact"][ns:], bound=att["bound"][ns:]), zero_S=False)
                if ws == "probe" and regime in ("integers", "mean50"):
                    m = l1["mean"]
                    assert out["v1_h"][0] == ish and out["v1_h"][1] == isw and bool((out["v1_h"][cin + 2:] == 0).all()), tag
                    _note(("mean", kl, regime), OC.worst(np.abs(out["v1_h"][2:cin + 2] - m["exact"]), m["bound"]))
                    assert bool((np.abs(out["v1_h"][2:cin + 2] - m["exact"]) <= m["bound"]).all()), tag
                    if regime == "integers":
                        assert np.array_equal(out["v1_h"][2:cin + 2], (p.astype(np.float64).sum(0).astype(F32) * inv_n).astype(F32)), tag
                if ws == "dead":
                    assert bool((out["v1_h"] == 0).all()) and np.array_equal(out["v2_h"], np.maximum(w["l2_b"], F32(0))), tag
                if ws == "sat":
                    r32 = att["exact"].astype(F32)
                    for v in (0.0, 1.0):
                        assert bool((out["att_h"][:ns][r32[:ns] == v] == v).all()), (tag, v)
                    if knum > 1:
                        assert float(out["att_h"][ns:].max()) > 1 - 1e-6, tag
                if ws == "uniform_k":
                    assert bool((out["att_h"][ns:] == F32(1.0) / F32(knum)).all()), tag
                if j == 0 and regime in ("gauss", "decades") and ws in IMAGE_SETS:
                    for wy in (False, True) if cout % 64 == 0 else (False,):
                        o = r.run(p, sc, inv_n, wy=True) if wy else out
                        assert not wy or np.array_equal(o["att_h"], out["att_h"]), tag
                        ref = OC.image_reference(w, o["att_h"], wy=wy, restate=False)
                        _check(tag + (" wy" if wy else " image"), ("wy" if wy else "image", kl, ws), r.decode(o["img"], wy), ref)
    print(f"{geom}: worst ratios of the bound so far: " + ", ".join(f"{'/'.join(k)} {v:.3f}" for k, v in sorted(WORST.items()) if k[1] == kl))


# ----------------------------------------------------------------------------- 2. fused == unfused
@pytest.mark.parametrize("geom", OC.GEOMS)
def test_fused_equals_unfused_bitwise(geom):
    """savsr_osconv_attn_desc.fused (one launch, the routing inside every aggregation workgroup) against the three-launch chain: v2, att and the
    image bit for bit, both image orders, every nblk; the scratch offset behind the gates takes every residue modulo 4 over the geometries."""
    cin, cout, hidden, knum = geom
    for ws in ("synth", "sat"):
        r = rig(ws, geom)
        for j, nblk in enumerate(OC.NBLKS):
            regime, sc = OC.REGIMES[j % 4], OC.SCALES[j % 2]
            p, inv_n = OC.partials(regime, nblk, cin), OC.inv_n_of(nblk)
            for wy in (False, True) if cout % 64 == 0 else (False,):
                a, b = r.run(p, sc, inv_n, wy=wy, fused=False), r.run(p, sc, inv_n, wy=wy, fused=True)
                for k in ("v2", "att", "img"):
                    assert torch.equal(_bits(a[k]), _bits(b[k])), (geom, ws, nblk, wy, k)
                assert not bool(torch.isnan(b["img"][:-GUARD]).any()), (geom, ws, nblk, wy)
                assert float(np.abs(b["v2_h"]).max()) > 0 or regime == "zero"


# ----------------------------------------------------------------------------- 3. the fp16 images
@pytest.mark.parametrize("geom", OC.GEOMS)
def test_f16_images_within_one_ulp(geom):
    """savsr_osconv_weights_batch_f16 at every geometry, fused and not: both images are the float64 entry from the launch's own gates within one
    fp16 ulp (the criterion of test_gpu_precision.py), on the synth and on the cancelling (`uniform_k`) banks; unaddressed entries are zero."""
    cin, cout, hidden, knum = geom
    for ws in ("synth", "uniform_k"):
        r = rig(ws, geom)
        p, inv_n, sc = OC.partials("gauss", 33, cin), OC.inv_n_of(33), OC.SCALES[0]
        for wy in (False, True) if cout % 64 == 0 else (False,):
            outs = [r.run(p, sc, inv_n, wy=wy, fused=fused, f16=True) for fused in (False, True)]
            assert torch.equal(_bits(outs[0]["img"]), _bits(outs[1]["img"])) and np.array_equal(outs[0]["att_h"], outs[1]["att_h"])
            ref = OC.image_reference(r.w, outs[0]["att_h"], wy=wy, restate=False)["exact"]
            got = r.decode(outs[0]["img"], wy, f16=True)
            ulp = np.spacing(np.abs(ref).astype(np.float16)).astype(np.float64)
            d = float((np.abs(got - ref) / ulp).max())
            print(f"{geom} {ws} {'wy' if wy else 'direct'} fp16 image: max {d:.3f} ulp [worst {_note(('f16', _klass(geom), ws), d):.3f}]")
            assert d <= 1.0


# ----------------------------------------------------------------------------- 4. batches
@pytest.mark.parametrize("geom", [(64, 64, 16, 8), (320, 64, 20, 8), (32, 64, 7, 11), (16, 1, 5, 2)])
@pytest.mark.parametrize("n", [8, 3])
def test_batch_equals_solo_bitwise(geom, n):
    """n descriptors with different partials, nblk, scales and outputs in one launch: each equals its solo launch bit for bit."""
    cin, cout, hidden, knum = geom
    r = rig("synth", geom)
    assert r.lib.savsr_osconv_weights_max_batch() == 8
    for wy in (False, True) if cout % 64 == 0 else (False,):
        for fused in (False, True):
            cases = [(OC.REGIMES[i % 4 if i % 4 != 3 else 6], OC.NBLKS[i % 5], ((1.5 + 0.3 * i, 4 - 0.2 * i))) for i in range(n)]
            parts = [_dev(OC.partials(reg, nblk, cin)) for reg, nblk, _ in cases]
            bufs = [r.out_bufs(wy) for _ in range(n)]
            descs = [r.desc(parts[i], cases[i][2], OC.inv_n_of(cases[i][1]), bufs[i], wy, fused) for i in range(n)]
            r._lib.check(r.launch(descs), "batch")
            for i in range(n):
                got = r.finish(bufs[i], fused)
                solo = r.run(OC.partials(cases[i][0], cases[i][1], cin), cases[i][2], OC.inv_n_of(cases[i][1]), wy=wy, fused=fused)
                for k in ("v1", "v2", "att", "img"):
                    assert torch.equal(_bits(got[k]), _bits(solo[k])), (geom, n, wy, fused, i, k)
            assert not torch.equal(_bits(bufs[0]["att"]), _bits(bufs[1]["att"]))


# ----------------------------------------------------------------------------- 5. refusals
def test_refusals_write_nothing():
    from savsr_amd import _lib
    geom = (64, 64, 16, 8)
    r, r2, r32 = rig("synth", geom), rig("synth", (192, 64, 16, 8)), rig("synth", (32, 32, 16, 8))
    p = _dev(OC.partials("gauss", 33, 64))
    inv_n, sc = OC.inv_n_of(33), OC.SCALES[0]
    E_ARG, E_ALIGN = -1, -2

    def refused(rg, descs, bufs, code, word):
        rc = rg.launch(descs)
        msg = rg.lib.savsr_last_error()
        assert rc == code and word in msg, (rc, msg)
        for b in bufs:
            for k, v in b.items():
                assert bool(torch.isnan(v).all()), (word, k)

    bufs = [r.out_bufs() for _ in range(9)]
    refused(r, [r.desc(p, sc, inv_n, b) for b in bufs], bufs, E_ARG, b"batch size")
    b1, b2 = r.out_bufs(), r2.out_bufs()
    refused(r, [r.desc(p, sc, inv_n, b1), r2.desc(_dev(OC.partials("gauss", 33, 192)), sc, inv_n, b2)], [b1, b2], E_ARG, b"must share")
    b3 = dict(r32.out_bufs(), img=_nan(r32.elems * 4 // 3))
    refused(r32, [r32.desc(_dev(OC.partials("gauss", 33, 32)), sc, inv_n, b3, wy=True)], [b3], E_ARG, b"Winograd-y")
    for field in ("bank", "wimg_out", "partial"):
        b = r.out_bufs()
        d = r.desc(p, sc, inv_n, b)
        setattr(d, field, getattr(d, field) + 4)
        refused(r, [d], [b], E_ALIGN, b"16-byte aligned")
    for off in (-1, 1):
        b = r.out_bufs()
        d = r.desc(p, sc, inv_n, b)
        d.nunits += off
        refused(r, [d], [b], E_ARG, b"nunits")
    b = r.out_bufs()
    _lib.check(r.launch([r.desc(p, sc, inv_n, b)]), "the accepted launch")
    assert not bool(torch.isnan(b["img"][:-GUARD]).any())


# ----------------------------------------------------------------------------- 6. sharpness on the device
@pytest.mark.parametrize("defect", ["lo", "bank"])
def test_sharpness_edited_bank(defect):
    """The unmodified kernel on an edited bank, against the float64 reference of the UNEDITED weights: `lo` -- bank 0's entries of output channels
    0 .. 31 x input chunk 1 x tap 5 rounded to bf16 (what a lost lo half of that group does to bank 0); `bank` -- bank 7 zeroed for output channels
    0 .. 31.  Every dominated entry (moved > 2 bound) is outside the bound, at least 3 of them; every untouched entry is inside."""
    geom = (64, 64, 16, 8)
    r = rig("synth", geom)
    p, inv_n, sc = OC.partials("gauss", 33, 64), OC.inv_n_of(33), OC.SCALES[0]
    bank = r.w["bank"].copy()
    if defect == "lo":
        sl = (0, slice(0, 32), slice(16, 32), 1, 2)
        bank[sl] = torch.from_numpy(bank[sl].copy()).to(torch.bfloat16).float().numpy()
    else:
        bank[7, :32] = 0
    out = r.run(p, sc, inv_n, bank=r.pack_bank(bank))
    clean = r.run(p, sc, inv_n)
    assert np.array_equal(out["att_h"], clean["att_h"])
    ref = OC.image_reference(r.w, out["att_h"], restate=False)
    ca, fa, sa, ka = (x.astype(np.float64) for x in OC.split_att(out["att_h"], geom))
    gate = fa[:, None, None, None] * sa.reshape(1, 1, 3, 3) * ca[None, :, None, None]
    moved = np.abs((ka.reshape(-1, 1, 1, 1, 1) * (r.w["bank"].astype(np.float64) - bank.astype(np.float64))).sum(0) * gate)
    got = r.decode(out["img"])
    viol = np.abs(got - ref["exact"]) > ref["bound"]
    dom, untouched = moved > 2 * ref["bound"], moved == 0
    print(f"sharpness {defect}: dominated {int(dom.sum())}, violating {int(viol.sum())}, untouched {int(untouched.sum())} of {viol.size}")
    assert int(dom.sum()) >= 3 and bool(viol[dom].all())
    assert int(untouched.sum()) >= viol.size // 2 and not bool(viol[untouched].any())
    _check("sharpness, unedited bank", ("image", "network", "synth"), r.decode(clean["img"]), ref)


# ----------------------------------------------------------------------------- 7. the SE gate and its scale-residual pass
class SeRig:
    def __init__(self, c, cmid):
        from savsr_amd import _lib
        self.c, self.cmid, self.lib, self.check = c, cmid, _lib.load(), _lib.check
        self.check(self.lib.savsr_prepare_device(), "savsr_prepare_device")
        self.w = OC.se_weights(c, cmid)
        self.t = {k: _dev(v) for k, v in self.w.items()}

    def _w(self):
        return tuple(self.t[k].data_ptr() for k in ("w1", "b1", "w2", "b2"))

    def gate(self, pd, inv_n):
        g = _nan(self.c)
        self.check(self.lib.savsr_se_gate(pd.data_ptr(), pd.shape[0], float(inv_n), *self._w(), self.c, self.cmid, g.data_ptr(), _stream()), "se_gate")
        torch.cuda.synchronize()
        assert bool(torch.isnan(g[self.c:]).all())
        return g

    def pair(self, g, r, x):
        npx = r.numel() // self.c
        o = _nan(npx * self.c)
        self.check(self.lib.savsr_scale_residual(r.data_ptr(), g.data_ptr(), x.data_ptr(), o.data_ptr(), self.c, npx, _stream()), "scale_residual")
        torch.cuda.synchronize()
        return o

    def fused(self, pd, inv_n, r, x):
        npx = r.numel() // self.c
        o = _nan(npx * self.c)
        self.check(self.lib.savsr_se_scale_residual(pd.data_ptr(), pd.shape[0], float(inv_n), *self._w(), self.c, self.cmid, r.data_ptr(), x.data_ptr(),
                                                    o.data_ptr(), npx, _stream()), "se_scale_residual")
        torch.cuda.synchronize()
        return o


def _rx(c, npx, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(npx * c, generator=g).to(DEV), torch.randn(npx * c, generator=g).to(DEV)


def _check_scaled(tag, out, gate, r, x, c):
    """out = r g + x within two roundings, from the kernel's own gate; the guard behind it intact."""
    n = r.numel()
    assert bool(torch.isnan(out[n:]).all()), tag
    gd = gate[:c].double().repeat(n // c)
    prod = r.double() * gd
    exact = prod + x.double()
    ok = (out[:n].double() - exact).abs() <= U24 * (1 + U24) * prod.abs() + U24 * exact.abs()
    assert bool(ok.all()), tag


@pytest.mark.parametrize("c,cmid", OC.SE_GEOMS)
def test_se_gate_and_scale_residual(c, cmid):
    """savsr_se_gate against float64 with the derived bound at every nblk and regime (cmid = 9: the second-layer loop beyond 8; cmid = 20: first-layer
    rows beyond the 16 waves); savsr_se_scale_residual == savsr_se_gate + savsr_scale_residual bit for bit, and r g + x within two roundings."""
    s = SeRig(c, cmid)
    r, x = _rx(c, 37, c + cmid)
    for nblk in OC.SE_NBLKS:
        for regime in ("gauss", "mean50", "altsign", "zero", "lastblock", "decades"):
            p, inv_n = OC.partials(regime, nblk, c), OC.inv_n_of(nblk)
            pd = _dev(p)
            g = s.gate(pd, inv_n)
            ref = OC.se_reference(s.w, p, inv_n)
            tag = f"se ({c}, {cmid}) nblk {nblk} {regime}"
            _check(tag, ("se_gate", f"{c}/{cmid}", regime), g[:c].cpu().numpy(), ref, zero_S=False)
            o1, o2 = s.pair(g, r, x), s.fused(pd, inv_n, r, x)
            assert torch.equal(_bits(o1), _bits(o2)), tag
            _check_scaled(tag, o2, g, r, x, c)
    print(f"se ({c}, {cmid}): worst ratio of the gate's bound " + ", ".join(f"{k[2]} {v:.3f}" for k, v in sorted(WORST.items()) if k[:2] == ("se_gate", f"{c}/{cmid}")))


@pytest.mark.parametrize("c,cmid,npx", [(64, 4, 70000), (128, 8, 40000)])
def test_se_scale_residual_tail_loop(c, cmid, npx):
    """More float4 elements than 4 x 256 x 1024 (1.12 M and 1.28 M, the first not a multiple of 1024): the loop behind the unrolled part."""
    s = SeRig(c, cmid)
    assert npx * c // 4 > 4 * 256 * 1024
    r, x = _rx(c, npx, npx)
    p, inv_n = OC.partials("gauss", 230, c), OC.inv_n_of(230)
    pd = _dev(p)
    g = s.gate(pd, inv_n)
    o1, o2 = s.pair(g, r, x), s.fused(pd, inv_n, r, x)
    assert torch.equal(_bits(o1), _bits(o2))
    _check_scaled(f"tail loop c {c}", o2, g, r, x, c)


@pytest.mark.parametrize("c,cmid", [(64, 4), (32, 2), (128, 20)])
def test_se_scale_residual_batch_strides(c, cmid):
    """savsr_se_scale_residual_batch, nclip = 3: partials, r, x and out at their own strides (gaps NaN); each clip equals its solo launch bit for bit
    and nothing is written into the gaps."""
    s = SeRig(c, cmid)
    npx, nblk, nclip = 53, 17, 3
    inv_n = OC.inv_n_of(nblk)
    ps, pr = nblk * c + 8, npx * c + 12
    part = torch.full((nclip * ps,), NAN, device=DEV)
    rr, xx, out = (torch.full((nclip * pr + GUARD,), NAN, device=DEV) for _ in range(3))
    solo = []
    for b in range(nclip):
        p = OC.partials(OC.REGIMES[b], nblk, c)
        r, x = _rx(c, npx, 10 * c + b)
        part[b * ps:b * ps + nblk * c] = _dev(p).reshape(-1)
        rr[b * pr:b * pr + npx * c], xx[b * pr:b * pr + npx * c] = r, x
        solo.append(s.fused(_dev(p), inv_n, r, x)[:npx * c])
    s.check(s.lib.savsr_se_scale_residual_batch(part.data_ptr(), nblk, float(inv_n), *s._w(), c, cmid, rr.data_ptr(), xx.data_ptr(), out.data_ptr(), npx, nclip,
                                                4 * ps, 4 * pr, 4 * pr, 4 * pr, _stream()), "se_scale_residual_batch")
    torch.cuda.synchronize()
    for b in range(nclip):
        assert torch.equal(_bits(out[b * pr:b * pr + npx * c]), _bits(solo[b])), b
        assert bool(torch.isnan(out[b * pr + npx * c:(b + 1) * pr]).all()), b
    assert bool(torch.isnan(out[nclip * pr:]).all())
    assert not torch.equal(_bits(solo[0]), _bits(solo[1]))


# ----------------------------------------------------------------------------- 8. channel sums
SUM_SHAPES = ((1, 1), (127, 1), (129, 1), (10, 8), (1000, 7))


@pytest.mark.parametrize("src_ch", [16, 32, 64])
def test_channel_sums(src_ch):
    """savsr_channel_sums, 1 .. 5 sources that are channel slices of one wider tensor whose other channels are NaN: every block's sums against
    float64 within gamma(ceil(per / PL) + PL) S, integer data bit for bit, empty trailing blocks zero, rows of `partial` beyond nblk untouched."""
    from savsr_amd import _lib
    lib = _lib.load()
    _lib.check(lib.savsr_prepare_device(), "savsr_prepare_device")
    for nsrc in range(1, 6):
        pix, ctot = nsrc * (src_ch + 4), nsrc * src_ch
        for npx, nblk in SUM_SHAPES:
            for kind in ("gauss", "integers"):
                g = np.random.RandomState([src_ch, nsrc, npx, nblk])
                data = (g.standard_normal((npx, ctot)) * 10.0 ** g.uniform(-2, 2, (1, ctot)) if kind == "gauss" else g.randint(-500, 500, (npx, ctot))).astype(F32)
                wide = torch.full((npx, pix), NAN, device=DEV)
                for sidx in range(nsrc):
                    wide[:, sidx * (src_ch + 4) + 4:(sidx + 1) * (src_ch + 4)] = _dev(data[:, sidx * src_ch:(sidx + 1) * src_ch])
                ptrs = (_lib.fptr * nsrc)(*[wide.data_ptr() + 4 * (sidx * (src_ch + 4) + 4) for sidx in range(nsrc)])
                pixs = (C.c_int32 * nsrc)(*[pix] * nsrc)
                part = torch.full((nblk + 2, ctot), NAN, device=DEV)
                _lib.check(lib.savsr_channel_sums(ptrs, pixs, nsrc, src_ch, npx, nblk, part.data_ptr(), _stream()), "channel_sums")
                torch.cuda.synchronize()
                assert bool(torch.isnan(part[nblk:]).all())
                got = part[:nblk].cpu().numpy().astype(np.float64)
                ref = OC.sums_reference(data, nblk)
                bound = OC.gamma(ref["depth"](src_ch)) * ref["S"]
                tag = f"channel_sums {nsrc} x {src_ch}, {npx} px in {nblk} blocks, {kind}"
                e = np.abs(got - ref["exact"])
                _note(("sums", str(src_ch), kind), OC.worst(e, bound))
                assert bool(np.isfinite(got).all()) and bool((e <= bound).all()), (tag, OC.worst(e, bound))
                if kind == "integers":
                    assert np.array_equal(got, ref["exact"]), tag
                if (npx, nblk) == (10, 8):
                    assert bool((got[5:] == 0).all()), tag
    print(f"channel_sums src_ch {src_ch}: worst ratio of the bound gauss {WORST[('sums', str(src_ch), 'gauss')]:.3f}")
