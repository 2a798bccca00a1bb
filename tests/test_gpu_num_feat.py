"""num_feat = 32 on the GPU: the width-generic SATU kernels (savsr_satu_nf_lr_stage / savsr_satu_nf_hr) against float64 references built
from the oracle's pieces, their C = 64 instantiation against the tuned kernels, and the whole network of a 32-wide checkpoint against the
REFERENCE's golden outputs (tests/golden/num_feat_outputs.npz), the CPU oracle, the batched flow and the YAML surface."""
import os

import numpy as np
import pytest
import torch

from oracle import savsr_oracle as O
from savsr_amd.utils import synth
from tests.golden_cases import rnd
from tests.num_feat_cases import NUM_FEAT_CASES
from tests.test_num_feat import lr_planes_float64, p32_float64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def _sd(nf, seed=3):
    from savsr_amd.archs.savsr_arch import SAVSR
    return synth.synth_state_dict(synth.manifest_of(SAVSR(num_feat=nf).state_dict()), seed=seed)


def _engine(sd, nf):
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.engine import HipEngine
    return HipEngine(sd, SAVSR(num_feat=nf).cfg, DEV)


@pytest.fixture(scope="module")
def sd32():
    return _sd(32)


@pytest.fixture(scope="module")
def e32(sd32):
    return _engine(sd32, 32)


def cl(x):
    return x.permute(1, 2, 0).contiguous().to(DEV)


def _record_float64(sd, nf, x, st):
    """LRcat [h][w][64 + nf/2] in savsr_satu_lr_stage_tail's row order: (A | B) rows acc_row(r, hh) at 32 hh + (0 | 16) + r, C-stack at 64."""
    a, b, cs = (t[0].permute(1, 2, 0) for t in lr_planes_float64(sd, nf, x, st))
    rec = torch.empty(x.shape[2], x.shape[3], 64 + nf // 2, dtype=torch.float64)
    for hh in range(2):
        for r in range(16):
            row = (r & 3) + 8 * (r >> 2) + 4 * hh
            rec[..., 32 * hh + r] = a[..., row]
            rec[..., 32 * hh + 16 + r] = b[..., row]
    rec[..., 64:] = cs
    return rec


@pytest.mark.parametrize("h,w", [(12, 14), (180, 320)])
def test_lr_record_vs_float64(e32, sd32, h, w):
    x = rnd((1, 32, h, w), 81, 1.0)
    st = rnd((1, 32, h, w), 82, 0.6)
    e32._select((7, 3, h, w), (4, 4))
    lrcat = e32.buf("satu.lrcat_nf", h, w, e32.satu_nf_rec)
    lrcat.fill_(float("nan"))                                       # every float of every record is written
    xd, sd_ = cl(x[0]), cl(st[0])
    e32.satu_nf_lr(e32.full(xd), e32.full(sd_), w, h, w)
    torch.cuda.synchronize()
    got = lrcat.cpu().double()
    assert bool(torch.isfinite(got).all())
    ref = _record_float64(sd32, 32, x, st)
    err, mag = float((got - ref).abs().max()), float(ref.abs().max())
    print(h, w, "LR record max-abs", err, "magnitude", mag)
    assert err < 2e-5 * max(1.0, mag)


def _p27(e, nf, x, st, sc, pad=20, poison_lr=True):
    _, _, h, w = x.shape
    H, W = O.get_hw(h, w, sc)
    e._select((7, 3, h, w), sc)
    if poison_lr:
        e.buf("satu.lrcat_nf", h, w, e.satu_nf_rec).fill_(float("nan"))
    p27 = torch.full((27, H * W + pad), float("nan"), device=DEV)
    xd, sd_ = cl(x[0]), cl(st[0])
    lrcat = e.satu_nf_lr(e.full(xd), e.full(sd_), w, h, w)
    e.satu_nf_hr(lrcat, h, w, sc, p27, H * W + pad)
    torch.cuda.synchronize()
    assert bool(torch.isnan(p27[:, H * W:]).all()), "nothing is written between the planes"
    return p27[:, :H * W].reshape(27, H, W).cpu().double()


@pytest.mark.parametrize("h,w,sc", [(6, 7, (4, 4)), (7, 6, (1.5, 4)), (5, 6, (3.7, 3.7)), (6, 5, (2.95, 3.75)), (13, 17, (2.7, 3.3))])
def test_p27_vs_float64(e32, sd32, h, w, sc):
    x = rnd((1, 32, h, w), 21, 1.0)
    st = rnd((1, 32, h, w), 22, 0.6)
    got = _p27(e32, 32, x, st, sc)
    ref = p32_float64(sd32, 32, x, st, sc)[:27]
    err = float((got - ref).abs().max())
    print(sc, "P max-abs", err, "magnitude", float(ref.abs().max()))
    assert err < 2e-5


def test_p27_large_offsets_and_borders(sd32):
    """Offsets of several LR pixels push taps outside the image (zeros padding); a 19 x 23 frame at x3.9 has a phase table of more than
    256 entries, so the HR stage reads the per-pixel expansion."""
    sd = dict(sd32)
    for k in ("upsample.offset.weight", "upsample.st_offset.weight"):
        sd[k] = sd[k] * 6.0
    e2 = _engine(sd, 32)
    for (h, w, sc) in [(9, 8, (4, 4)), (9, 8, (2.5, 1.3)), (19, 23, (3.9, 3.9))]:
        x = rnd((1, 32, h, w), 31, 1.0)
        st = rnd((1, 32, h, w), 32, 0.6)
        got = _p27(e2, 32, x, st, sc)
        ax = e2.satu_axes(h, w, sc)
        if (h, w) == (19, 23):
            assert ax["n_uh"] * ax["n_uw"] > 256 and ax["ptab"] is not None
        ref = p32_float64(sd, 32, x, st, sc)[:27]
        err = float((got - ref).abs().max())
        print("large offsets", (h, w, sc), err)
        assert err < 5e-5


def test_c64_instantiation_equals_the_tuned_kernels(synth_sd):
    """The width-generic kernels at C = 64 (cross-check instantiation) against savsr_satu_lr_stage_tail + savsr_satu_hr_tail on identical
    inputs: same record layout, same planes."""
    from savsr_amd import _lib
    e = _engine(synth_sd, 64)
    e._pack_satu_nf(synth_sd, 64)
    e.satu_nf_rec = int(e.lib.savsr_satu_nf_lrcat_floats(64))
    for (h, w, sc) in [(13, 16, (4, 4)), (17, 21, (1.5, 4)), (12, 14, (3.7, 3.7))]:
        x = rnd((1, 64, h, w), 41, 1.0)
        st = rnd((1, 64, h, w), 42, 0.6)
        H, W = O.get_hw(h, w, sc)
        e._select((7, 3, h, w), sc)
        xd, sd_ = cl(x[0]), cl(st[0])
        tuned_rec = e.satu_lr(e.full(xd), e.full(sd_), w, h, w, tail_form=True)
        nf_rec = e.satu_nf_lr(e.full(xd), e.full(sd_), w, h, w)
        p_t = torch.full((27, H * W), float("nan"), device=DEV)
        p_n = torch.full((27, H * W), float("nan"), device=DEV)
        e.satu_hr(tuned_rec, h, w, sc, p_t, tail_form=True)
        e.satu_nf_hr(nf_rec, h, w, sc, p_n)
        p_x = torch.full((27, H * W), float("nan"), device=DEV)
        e.satu_nf_hr(tuned_rec, h, w, sc, p_x)                  # the tuned record through the generic HR stage
        torch.cuda.synchronize()
        assert tuned_rec.shape[-1] == nf_rec.shape[-1] == _lib.SATU_LRCAT_TAIL
        er = float((tuned_rec - nf_rec).abs().max())
        ep = float((p_t - p_n).abs().max())
        ex = float((p_t - p_x).abs().max())
        print((h, w, sc), "record", er, "planes", ep, "tuned record -> generic HR", ex)
        assert er < 2e-5 and ep < 2e-5 and ex < 1e-5


def _net32(sd, cfg):
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR(**cfg)
    net.load_state_dict(sd, strict=True)
    return net.to(DEV).eval()


@pytest.mark.parametrize("name,cfg,h,w,sc", NUM_FEAT_CASES)
def test_network_vs_reference_golden(name, cfg, h, w, sc):
    """A 32-wide checkpoint end to end: within 5e-5 max-abs of the reference's output; eager, captured and replayed runs bitwise equal."""
    gold = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "num_feat_outputs.npz"))[f"{name}/sr"])
    from savsr_amd.archs.savsr_arch import SAVSR
    net = _net32(synth.synth_state_dict(synth.manifest_of(SAVSR(**cfg).state_dict()), seed=3), cfg)
    net.set_scale(sc)
    lq = synth.synth_clip(cfg.get("num_frame", 7), 3, h, w, seed=5).to(DEV)
    taps = {}
    eager = net(lq, taps=taps).cpu()                     # taps force the eager launch sequence
    a = net(lq).cpu()                                    # captured
    b = net(lq).cpu()                                    # replayed
    assert "satu" not in taps and tuple(taps["p27"].shape[0:1]) == (27,)
    assert a.shape == gold.shape
    err = float((a - gold).abs().max())
    print(name, "max-abs vs reference", err)
    assert err < 5e-5
    assert torch.equal(a, b) and torch.equal(a, eager)


def test_network_64x96_x4_vs_oracle(sd32):
    net = _net32(sd32, dict(num_feat=32))
    net.set_scale((4, 4))
    lq = synth.synth_clip(7, 3, 64, 96, seed=9)
    out = net(lq.to(DEV)).cpu()
    with torch.no_grad():
        ref = O.forward(sd32, lq, (4, 4), cfg=dict(num_feat=32))
    err = float((out - ref).abs().max())
    print("64x96 x4 max-abs vs oracle", err)
    assert err < 5e-5


def test_forward_many_group_equals_one_clip_runs(sd32):
    """Clips of one (shape, scale) batched into one launch sequence: each result equals that clip's own run bit for bit."""
    net = _net32(sd32, dict(num_feat=32))
    clips = [synth.synth_clip(7, 3, 20, 24, seed=s)[0].to(DEV) for s in (1, 2, 3)]
    sc = (2.5, 3.5)
    group = net.forward_many(clips, [sc] * 3)
    for c, g in zip(clips, group):
        one = net.forward_many([c], [sc])[0]
        assert torch.equal(g, one)
    with torch.no_grad():
        ref = O.forward(sd32, clips[1].cpu().unsqueeze(0), sc, cfg=dict(num_feat=32))[0]
    assert float((group[1].cpu() - ref).abs().max()) < 5e-5


def test_num_feat_96_is_rejected_at_engine_build():
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR(num_feat=96)
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=0), strict=True)
    net = net.to(DEV).eval()
    net.set_scale((2, 2))
    with pytest.raises(RuntimeError, match=r"cin <= 320 and hidden <= 32"):
        net(synth.synth_clip(7, 3, 8, 8, seed=0).to(DEV))


def test_run_test_yaml_with_a_32_wide_checkpoint(tmp_path, sd32):
    """run_test on a synthetic PNG tree with a `num_feat: 32` YAML and a 32-wide .pth: the metric table is finite and one frame equals
    the CPU oracle's to a quantisation level (the pattern of test_gpu_run_test.py)."""
    from savsr_amd import io as sio
    from savsr_amd import metrics as M
    from savsr_amd.harness import window_indices
    from savsr_amd.options import parse_test_options
    from savsr_amd.resize_gpu import as_mod_crop_hw
    from savsr_amd.test import run_test
    from tests.test_gpu_run_test import YAML
    root = str(tmp_path)
    n, H, W = 5, 45, 62
    for i in range(n):
        sio.imwrite(M.tensor2img(synth.synth_gt(3, H, W, seed=40 + i)), os.path.join(root, "GT", "city", f"{i:08d}.png"))
    torch.save({"params": {k: v.clone() for k, v in sd32.items()}}, os.path.join(root, "savsr_synth.pth"))
    text = YAML.format(root=root).replace("num_feat: 64", "num_feat: 32")
    assert "num_feat: 32" in text
    opt = parse_test_options(text, root_path=root)
    results = run_test(opt)
    sc = (1.5, 2.5)
    r = results[1]
    assert r["scale"] == sc and set(r["folders"]) == {"city"}
    rows = r["frames"]["city"]
    assert tuple(rows.shape) == (n, 2) and bool(torch.isfinite(rows).all())
    Hc, Wc = as_mod_crop_hw(H, W, sc)
    gt = sio.read_img_seq(os.path.join(root, "GT", "city"), require_as_mod_crop=True, scale=sc)
    lq = torch.nn.functional.interpolate(gt, size=(round(Hc / sc[0]), round(Wc / sc[1])), mode="bicubic", align_corners=False, antialias=True)
    with torch.no_grad():
        ref = O.forward(sd32, lq[window_indices(1, n, 7)].unsqueeze(0), sc, cfg=dict(num_feat=32))
    want = M.tensor2img(ref[0])
    got = sio.imread(os.path.join(root, "results", opt["name"], "visualization", r["dataset"], "city", f"{1:08d}_{opt['name']}.png"))
    assert want.shape == got.shape
    d = np.abs(want.astype(np.int32) - got.astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 5e-3, (d.max(), (d > 0).mean())
    gtc = sio.imread(os.path.join(root, "GT", "city", f"{1:08d}.png"))[:Hc, :Wc]
    assert abs(M.calculate_psnr(got, gtc, 0, test_y_channel=True) - float(rows[1, 0])) < 1e-4
