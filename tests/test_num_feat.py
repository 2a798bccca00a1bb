"""num_feat = 32 checkpoints (the width-generic SATU, savsr_satu_nf_*), host side: the parameter tree and the oracle against the
REFERENCE's outputs (tests/golden/num_feat_outputs.npz, tools/gen_golden_num_feat.py), the record-size query of the C ABI, and the
float64 algebra of the folded SATU matrices (packing.fold_satu_nf) against the oracle's STAUpsample + tail conv."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import savsr_oracle as O
from savsr_amd.utils import synth
from tests.golden_cases import manifest_hash, rnd
from tests.num_feat_cases import NUM_FEAT_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nfgold():
    return np.load(os.path.join(ROOT, "tests", "golden", "num_feat_outputs.npz"))


def _net(cfg):
    from savsr_amd.archs.savsr_arch import SAVSR
    return SAVSR(**cfg)


@pytest.mark.parametrize("name,cfg,h,w,sc", NUM_FEAT_CASES)
def test_parameter_tree_matches_the_reference(nfgold, name, cfg, h, w, sc):
    manifest = synth.manifest_of(_net(cfg).state_dict())
    assert len(manifest) == int(nfgold[f"{name}/n_keys"][0])
    assert manifest_hash(manifest) == bytes(nfgold[f"{name}/manifest_sha"]).hex()


@pytest.mark.parametrize("name,cfg,h,w,sc", NUM_FEAT_CASES)
def test_oracle_vs_reference_golden(nfgold, name, cfg, h, w, sc):
    sd = synth.synth_state_dict(synth.manifest_of(_net(cfg).state_dict()), seed=3)
    lq = synth.synth_clip(cfg.get("num_frame", 7), 3, h, w, seed=5)
    with torch.no_grad():
        sr = O.forward(sd, lq, sc, cfg=cfg)
    gold = torch.from_numpy(nfgold[f"{name}/sr"])
    assert sr.shape == gold.shape
    assert float((sr - gold).abs().max()) <= 1e-6


def test_lrcat_record_size_query():
    from savsr_amd import _lib
    lib = _lib.load()
    assert lib.savsr_satu_nf_lrcat_floats(32) == 80
    assert lib.savsr_satu_nf_lrcat_floats(64) == 96 == _lib.SATU_LRCAT_TAIL
    for c in (48, 96, 256, 0, -32):
        assert lib.savsr_satu_nf_lrcat_floats(c) == -1


def test_unsupported_widths_name_their_limit():
    from savsr_amd.engine import HipEngine
    for nf in (96, 128):
        msg = HipEngine.num_feat_limit(nf)
        assert "cin <= 320" in msg and "hidden <= 32" in msg and "OSConv" in msg, msg
    assert "32" in HipEngine.num_feat_limit(48) and "64" in HipEngine.num_feat_limit(48)


def _grid_sample64(x, offset, scale):
    """satu_grid_sample (savsr_arch.py:262-295) with the reference's fp32 grid, sampling a float64 tensor."""
    b, _, h, w = x.shape
    H, W = O.get_hw(h, w, scale)
    g = torch.Tensor(np.stack(np.meshgrid(range(W), range(H)), axis=-1).astype(np.float64))
    g[:, :, 0] = (g[:, :, 0] + 0.5) / scale[1] - 0.5
    g[:, :, 1] = (g[:, :, 1] + 0.5) / scale[0] - 0.5
    g[:, :, 0] = g[:, :, 0] * 2 / (w - 1) - 1
    g[:, :, 1] = g[:, :, 1] * 2 / (h - 1) - 1
    g = g.permute(2, 0, 1).unsqueeze(0)
    o0 = torch.unsqueeze(offset[:, 0] * 2 / (w - 1), dim=1)
    o1 = torch.unsqueeze(offset[:, 1] * 2 / (h - 1), dim=1)
    g = (g + torch.cat((o0, o1), 1)).permute(0, 2, 3, 1)
    return F.grid_sample(x, g.double(), mode="bilinear", padding_mode="zeros", align_corners=True)


def lr_planes_float64(sd, nf, x, st, row_of=None):
    """float64 LR side of the tail-projected SATU from fold_satu_nf's products: (Wt27 Wa sta [32], Wt27 Wb x [32], C-stack x [nf/2]),
    each [1][rows][h][w].  x, st: [1][nf][h][w]; row_of: the row order of Wt27 (default: the 27-plane forms')."""
    from savsr_amd.packing import fold_satu_nf
    m = fold_satu_nf(sd, nf, row_of)
    _, _, h, w = x.shape
    x64, st64 = x[0].double().reshape(nf, -1), st[0].double().reshape(nf, -1)
    k = torch.from_numpy(m["kconv"]) @ st64 + torch.from_numpy(m["kconv_b"])[:, None]
    k = torch.where(k > 0, k, 0.1 * k)                                                           # :227
    sta = O.sta_conv(x[0:1].double(), k.reshape(1, 25 * nf, h, w))[0].reshape(nf, -1)          # :297-313
    return ((torch.from_numpy(m["ta"]) @ sta).reshape(1, 32, h, w), (torch.from_numpy(m["tb"]) @ x64).reshape(1, 32, h, w),
            (torch.from_numpy(m["cstack"]) @ x64).reshape(1, nf // 2, h, w))


def p32_float64(sd, nf, x, st, sc, row_of=None):
    """The 32 tail-projected planes P (rows 27 .. 31 zero) in float64: two bilinear gathers of the LR planes, expert mixing, Wt27 b."""
    from savsr_amd.packing import fold_satu_nf
    m = fold_satu_nf(sd, nf, row_of)
    _, _, h, w = x.shape
    H, W = O.get_hw(h, w, sc)
    with torch.no_grad():
        off, soff, r = O.satu_heads(sd, "upsample", h, w, sc)
    a, b, cs = lr_planes_float64(sd, nf, x, st, row_of)
    ga, gb, gc = _grid_sample64(a, soff, sc)[0], _grid_sample64(b, off, sc)[0], _grid_sample64(cs, off, sc)[0]
    rr = r[0].double()                                                           # [4][H][W]
    J = nf // 8
    z = sum(rr[mi] * gc[mi * J:(mi + 1) * J] for mi in range(4))                 # [J][H][W]
    u = torch.stack([rr[n] * z for n in range(4)], 0).reshape(4 * J, H, W)      # (n, j)
    wbe = torch.from_numpy(m["wbe"]).reshape(4 * J, 32)
    return torch.from_numpy(m["fb"])[:, None, None] + ga + gb + torch.einsum("qp,qhw->phw", wbe, u)


@pytest.mark.parametrize("nf,h,w,sc", [(32, 7, 9, (4, 4)), (32, 6, 8, (2.7, 1.6)), (64, 5, 7, (3.5, 2))])
def test_folded_nf_matrices_reproduce_satu_and_tail_conv(nf, h, w, sc):
    """The float64 products fold_satu_nf hands to the packer (before the fp32 rounding and the bf16 split), evaluated the way the kernels
    evaluate them -- LR record (Wt27 Wa sta | Wt27 Wb x | C-stack x), two bilinear gathers, expert mixing, the nine shifted taps --
    equal the oracle's STAUpsample followed by the 3x3 tail conv."""
    sd = synth.synth_state_dict(synth.manifest_of(_net(dict(num_feat=nf)).state_dict()), seed=4)
    x = rnd((1, nf, h, w), 71, 1.0)
    st = rnd((1, nf, h, w), 72, 0.6)
    with torch.no_grad():
        ref = F.conv2d(O.sta_upsample(sd, "upsample", x, sc, st), sd["tail.weight"], sd["tail.bias"], padding=1)[0].double()
    H, W = O.get_hw(h, w, sc)
    p = p32_float64(sd, nf, x, st, sc)
    assert float(p[27:].abs().max()) == 0.0
    pp = F.pad(p[:27], (1, 1, 1, 1))
    out = sd["tail.bias"].double()[:, None, None].repeat(1, H, W)
    for ky in range(3):
        for kx in range(3):
            for o in range(3):
                out[o] += pp[3 * (3 * ky + kx) + o, ky:ky + H, kx:kx + W]
    err = float((out - ref).abs().max())
    print(nf, sc, "folded float64 vs oracle", err, "magnitude", float(ref.abs().max()))
    assert err <= 1e-5
