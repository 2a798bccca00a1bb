"""tests/osconv_cases.py on the CPU: its float64 references against the oracle, what its weight sets and regimes promise, its fp32
restatements of the kernels' summation orders inside every bound, and the sharpness of the bounds -- simulated defects in the restatements
violate them in the elements the defect dominates and in no element it does not touch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import savsr_oracle as O
from tests import osconv_cases as OC
from tests.golden_cases import OSCONV_CASES, OSCONV_SCALES, rnd

F32 = np.float32


def chain32(w, partial, sc, inv_n):
    """The fp32 restatement stage by stage, each stage's reference evaluated on the restatement of the stage before (as the GPU tests
    evaluate it on what the launch wrote)."""
    ish, isw = OC.inv_scales(sc)
    l1 = OC.l1_reference(w, partial, ish, isw, inv_n)
    l2 = OC.l2_reference(w, l1["f32"])
    att = OC.att_reference(w, l2["f32"])
    return l1, l2, att


def _inside(ref, what):
    e = np.abs(ref["f32"].astype(np.float64) - ref["exact"])
    assert bool((e <= ref["bound"]).all()), (what, OC.worst(e, ref["bound"]))
    return OC.worst(e, ref["bound"])


@pytest.mark.parametrize("tag,pfx,cin", OSCONV_CASES)
def test_references_reproduce_the_oracle(synth_sd, tag, pfx, cin):
    """synth state dict, 10 x 12: the chain of float64 references gives O.scale_attention's gates and, convolved in float64, O.osconv2d's
    output, to fp32 tolerance (the oracle runs in fp32)."""
    w = OC.from_state_dict(synth_sd, pfx)
    x = rnd((1, cin, 10, 12), 11 + cin, 0.7)
    partial = x[0].double().sum((1, 2)).float().numpy()[None]
    for sc in OSCONV_SCALES:
        ish, isw = OC.inv_scales(sc)
        l1 = OC.l1_reference(w, partial, ish, isw, F32(1.0 / 120))
        l2 = OC.l2_reference(w, l1["exact"].astype(F32))
        att = OC.att_reference(w, l2["exact"].astype(F32))
        with torch.no_grad():
            v = torch.cat([torch.tensor([[1.0 / sc[0], 1.0 / sc[1]]]), x.mean(dim=(2, 3))], 1)
            v = F.relu(F.linear(v, synth_sd[pfx + ".scale_routing.0.weight"], synth_sd[pfx + ".scale_routing.0.bias"]))
            v = F.relu(F.linear(v, synth_sd[pfx + ".scale_routing.2.weight"], synth_sd[pfx + ".scale_routing.2.bias"]))
            gates = O.scale_attention(synth_sd, pfx + ".attention", v.view(1, cin, 1, 1))
            ref = O.osconv2d(synth_sd, pfx, x, sc)[0].double()
        assert np.abs(l2["exact"] - v[0].double().numpy()).max() <= 2e-6
        assert np.abs(att["exact"] - torch.cat([t.reshape(-1) for t in gates]).double().numpy()).max() <= 2e-6
        img = OC.image_reference(w, att["exact"].astype(F32), restate=False)["exact"]
        got = F.conv2d(x.double(), torch.from_numpy(img), padding=1)[0]
        assert float((got - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))
        u = OC.image_reference(w, att["exact"].astype(F32), wy=True, restate=False)["exact"]
        from savsr_amd.packing import wy_transform_f64
        assert np.abs(u - wy_transform_f64(torch.from_numpy(img))).max() <= 1e-15


@pytest.mark.parametrize("geom", OC.GEOMS)
def test_weight_sets_deliver_what_they_promise(geom):
    cin, cout, hidden, knum = geom
    sc, nblk = OC.SCALES[0], 33
    inv_n = OC.inv_n_of(nblk)
    ish, isw = OC.inv_scales(sc)
    # probe: v1 = [inv_sh, inv_sw, mean] -- the scales bit for bit, the mean within its depth bound; integer partials: fl(sum inv_n) bit for bit
    w = OC.weights("probe", geom)
    for regime in ("integers", "mean50"):
        p = OC.partials(regime, nblk, cin)
        assert float(p.min()) > 0
        l1 = OC.l1_reference(w, p, ish, isw, inv_n)
        assert l1["f32"][0] == ish and l1["f32"][1] == isw and ish != isw
        m = l1["mean"]
        assert np.array_equal(l1["f32"][2:cin + 2], m["f32"]) and bool((l1["f32"][cin + 2:] == 0).all())
        assert bool((np.abs(m["f32"] - m["exact"]) <= m["bound"]).all())
        if regime == "integers":
            tot = p.astype(np.float64).sum(0)
            assert float(tot.max()) < 2 ** 24 and np.array_equal(m["f32"], (tot.astype(F32) * inv_n).astype(F32))
    # dead: v1 == 0 and v2 == max(l2_b, 0) bit for bit
    w = OC.weights("dead", geom)
    l1, l2, _ = chain32(w, OC.partials("mean50", nblk, cin), sc, inv_n)
    assert bool((l1["f32"] == 0).all()) and bool((l1["exact"] == 0).all())
    assert np.array_equal(l2["f32"], np.maximum(w["l2_b"], F32(0))) and bool((l2["f32"] > 0).any())
    # sat: saturated gates, a one-hot softmax, everything finite
    w = OC.weights("sat", geom)
    for regime in ("gauss", "mean50", "zero"):
        _, _, att = chain32(w, OC.partials(regime, nblk, cin), sc, inv_n)
        lg, ns = att["logit"], att["sig"]
        assert float(lg[:ns].max()) >= 100 and float(lg[:ns].min()) <= -100
        assert bool(np.isfinite(att["f32"]).all())
        r32 = att["exact"].astype(F32)
        for v in (0.0, 1.0):
            at = r32[:ns] == v
            assert bool(at.any()) and bool((att["f32"][:ns][at] == v).all()), v
        _inside(att, ("sat", regime))
        if knum > 1:
            assert float(lg[ns:].max() - lg[ns:].min()) > 100
            ka = att["f32"][ns:]
            assert float(ka.max()) > 1 - 1e-6 and float(np.sort(ka)[-2]) < 1e-6
        img = OC.image_reference(w, att["f32"], restate=False)
        assert bool((img["T"] == 0).any()) and bool((img["T"] > 0).any())
    # uniform_k: ka is fl(1 / K) and the aggregation cancels
    w = OC.weights("uniform_k", geom)
    _, _, att = chain32(w, OC.partials("gauss", nblk, cin), sc, inv_n)
    assert bool((att["f32"][att["sig"]:] == F32(1.0) / F32(knum)).all())
    if knum % 2 == 0:
        img = OC.image_reference(w, att["f32"], restate=False)
        assert float(np.median(np.abs(img["exact"]) / img["T"])) < 1e-3
    # decades: bank magnitudes over more than four decades
    mag = np.abs(OC.weights("decades", geom)["bank"]).mean((0, 3, 4))
    assert float(mag.max() / mag.min()) > (1e4 if cout > 1 else 1e2)


def test_partial_regimes_deliver_what_they_promise():
    for nblk in OC.NBLKS:
        c = 64
        p = {r: OC.partials(r, nblk, c) for r in OC.REGIMES}
        assert bool((p["zero"] == 0).all())
        assert bool((p["lastblock"][:nblk - 1] == 0).all()) and bool((p["lastblock"][nblk - 1] != 0).all())
        assert bool((p["integers"] == np.round(p["integers"])).all())
        if nblk > 1:
            assert bool((np.sign(p["altsign"][0]) != np.sign(p["altsign"][1])).all())
            m = OC.mean_reference(p["altsign"], OC.inv_n_of(nblk))
            assert float(np.median(np.abs(m["exact"]) / m["S"])) < (0.2 if nblk % 2 == 0 else 1.1)
        col = np.abs(p["decades"]).max(0)
        assert float(col.max() / col.min()) > 1e3
        assert OC.mean_reference(p["zero"], OC.inv_n_of(nblk))["S"].max() == 0
    assert sorted({OC.scratch_residue(g) for g in OC.GEOMS}) == [0, 1, 2, 3]
    assert all(OC.scratch_residue(g) == 1 for g in OC.NETWORK_GEOMS)
    assert max(OC.ngate(g) for g in OC.GEOMS) > 512


@pytest.mark.parametrize("geom", OC.GEOMS)
def test_restatements_meet_every_bound(geom):
    """The fp32 restatements -- the kernels' summation orders with every product rounded -- sit inside every bound, every weight set, every
    partial regime, every nblk."""
    cin, cout, hidden, knum = geom
    worst = {}
    for ws in OC.WEIGHT_SETS:
        w = OC.weights(ws, geom)
        for i, regime in enumerate(OC.REGIMES):
            for j, nblk in enumerate(OC.NBLKS):
                sc = OC.SCALES[(i + j) % 2]
                l1, l2, att = chain32(w, OC.partials(regime, nblk, cin), sc, OC.inv_n_of(nblk))
                for k, r in (("mean", l1["mean"]), ("v1", l1), ("v2", l2), ("att", att)):
                    worst[k] = max(worst.get(k, 0.0), _inside(r, (ws, regime, nblk, k)))
                assert bool((l1["f32"][l1["S"] == 0] == 0).all())
                if j == 0 and regime in ("gauss", "decades") and ws in ("synth", "sat", "uniform_k", "decades") and (cin * cout < 320 * 192 or regime == "gauss"):
                    for wy in (False, True) if cout % 64 == 0 else (False,):
                        img = OC.image_reference(w, att["f32"], wy=wy)
                        e = np.abs(img["f32"] - img["exact"])
                        k = "wy" if wy else "image"
                        assert bool((e <= img["bound"]).all()), (ws, regime, k, OC.worst(e, img["bound"]))
                        assert bool((img["f32"][img["T"] == 0] == 0).all())
                        worst[k] = max(worst.get(k, 0.0), OC.worst(e, img["bound"]))
    print(geom, {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values())


def _sharp(tag, got, ref, min_dom=3):
    viol = np.abs(got - ref["exact"]) > ref["bound"]
    dom, untouched = ref["moved"] > 2 * ref["bound"], ref["moved"] == 0
    print(f"{tag}: dominated {int(dom.sum())}, violating {int(viol.sum())}, untouched {int(untouched.sum())} of {viol.size}")
    assert int(dom.sum()) >= min_dom and bool(viol[dom].all()), tag
    assert not bool(viol[untouched].any()), tag


@pytest.mark.parametrize("geom", [(64, 64, 16, 8), (192, 64, 16, 8), (32, 64, 7, 11)])
def test_simulated_defects_violate_the_bounds_where_they_dominate(geom):
    cin, cout, hidden, knum = geom
    w = OC.weights("synth", geom)
    nblk = 33
    p, inv_n = OC.partials("mean50", nblk, cin), OC.inv_n_of(nblk)
    ish, isw = OC.inv_scales((1.5, 4))
    for defect in (("lastcol",), ("swap",)):
        r = OC.l1_reference(w, p, ish, isw, inv_n, defect=defect)
        _sharp(f"{geom} L1 {defect}", r["f32"].astype(np.float64), r)
    eq = OC.inv_scales((3.7, 3.7))
    r = OC.l1_reference(w, p, *eq, inv_n, defect=("swap",))      # equal scales: the swap is no defect
    assert bool((r["moved"] == 0).all()) and bool((np.abs(r["f32"] - r["exact"]) <= r["bound"]).all())
    _, _, att = chain32(w, OC.partials("gauss", nblk, cin), (1.5, 4), inv_n)
    for defect in (("lo", 1, 5), ("lo", 0, 0), ("bank", knum - 1), ("bank", 0), ("sa_t",)):
        r = OC.image_reference(w, att["f32"], defect=defect)
        _sharp(f"{geom} image {defect}", r["f32"], r)
        if defect[0] == "sa_t":
            diag = np.zeros(r["moved"].shape, dtype=bool)
            diag[:, :, [0, 1, 2], [0, 1, 2]] = True
            assert bool((r["moved"][diag] == 0).all()) and bool((r["moved"][~diag] > 0).any())


def test_se_gate_and_sums_references():
    """The SE gate's restatement inside its bound at every (c, cmid, nblk); a missing last input column or hidden unit is outside."""
    for c, cmid in OC.SE_GEOMS:
        w = OC.se_weights(c, cmid)
        for nblk in OC.SE_NBLKS:
            for regime in ("gauss", "mean50", "altsign", "zero"):
                r = OC.se_reference(w, OC.partials(regime, nblk, c), OC.inv_n_of(nblk))
                assert bool((np.abs(r["f32"] - r["exact"]) <= r["bound"]).all()), (c, cmid, nblk, regime)
                assert bool((r["exact"] >= 0).all()) and bool((r["exact"] <= 1).all())
        p = OC.partials("mean50", 17, c)
        r = OC.se_reference(w, p, OC.inv_n_of(17))
        w_bad = dict(w, w2=w["w2"].copy())
        w_bad["w2"][:, cmid - 1] = 0
        bad = OC.se_reference(w_bad, p, OC.inv_n_of(17))["f32"]
        moved = np.abs(bad.astype(np.float64) - r["exact"])
        if bool((moved > 4 * r["bound"]).any()):
            assert bool((np.abs(bad - r["exact"]) > r["bound"])[moved > 4 * r["bound"]].all())
    x = OC.partials("gauss", 10, 32)
    s = OC.sums_reference(x, 8)
    assert s["per"] == 2 and bool((s["exact"][5:] == 0).all()) and s["depth"](32) == 1 + 32
    assert np.allclose(s["exact"].sum(0), x.astype(np.float64).sum(0))
