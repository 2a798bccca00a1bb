"""num_in_ch / slid_win checkpoints beside the shipped 3 / 3, host side: the parameter tree and the oracle against the REFERENCE's outputs
(tests/golden/channels_outputs.npz, tools/gen_golden_channels.py), the fused window conv (packing.fuse_window_conv) against conv_c /
conv_sup, the nch-row SATU / tail fold (packing.fold_satu_nf) against STAUpsample + the tail conv, and the engine's refusals."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import savsr_oracle as O
from savsr_amd.utils import synth
from tests.channel_cases import CHANNEL_CASES
from tests.golden_cases import manifest_hash, rnd
from tests.test_num_feat import p32_float64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def chgold():
    return np.load(os.path.join(ROOT, "tests", "golden", "channels_outputs.npz"))


def _net(cfg):
    from savsr_amd.archs.savsr_arch import SAVSR
    return SAVSR(**cfg)


def _cfg(**kw):
    from savsr_amd.archs.savsr_arch import SAVSR
    c = dict(SAVSR().cfg)
    c.update(kw)
    return c


def pack_windows_ref(lq: torch.Tensor, sw: int) -> torch.Tensor:
    """What savsr_pack_windows_nch writes, in torch: lq [T][nch][h][w] -> [T-sw+1][hp][wp][RW] channel-last (pad_spatial's reflect padding,
    savsr_arch.py:670-690; window centre t = q + sw // 2, centre frame first, then the support frames ascending, :448-454; zeros to RW)."""
    from savsr_amd.packing import window_record
    T, nch, h, w = lq.shape
    x = F.pad(lq.reshape(1, T * nch, h, w), [0, w & 1, 0, h & 1], mode="reflect")[0].reshape(T, nch, h + (h & 1), w + (w & 1))
    rw = window_record(nch, sw)
    out = torch.zeros(T - sw + 1, x.shape[2], x.shape[3], rw, dtype=lq.dtype)
    half = sw // 2
    for q in range(T - sw + 1):
        t = q + half
        frames = [t] + [t - half + i for i in range(sw) if i != half]
        out[q, :, :, :nch * sw] = x[frames].reshape(nch * sw, x.shape[2], x.shape[3]).permute(1, 2, 0)
    return out


@pytest.mark.parametrize("name,cfg,h,w,sc", CHANNEL_CASES)
def test_parameter_tree_matches_the_reference(chgold, name, cfg, h, w, sc):
    manifest = synth.manifest_of(_net(cfg).state_dict())
    assert len(manifest) == int(chgold[f"{name}/n_keys"][0])
    assert manifest_hash(manifest) == bytes(chgold[f"{name}/manifest_sha"]).hex()


@pytest.mark.parametrize("name,cfg,h,w,sc", CHANNEL_CASES)
def test_oracle_vs_reference_golden(chgold, name, cfg, h, w, sc):
    sd = synth.synth_state_dict(synth.manifest_of(_net(cfg).state_dict()), seed=3)
    lq = synth.synth_clip(cfg.get("num_frame", 7), cfg.get("num_in_ch", 3), h, w, seed=5)
    nt = torch.get_num_threads()
    torch.set_num_threads(8)                     # (the goldens' thread count: the oracle's reductions follow it)
    try:
        with torch.no_grad():
            sr = O.forward(sd, lq, sc, cfg=cfg)
    finally:
        torch.set_num_threads(nt)
    gold = torch.from_numpy(chgold[f"{name}/sr"])
    assert sr.shape == gold.shape == (1, cfg.get("num_in_ch", 3)) + O.get_hw(h, w, sc)
    assert float((sr - gold).abs().max()) <= 1e-6


@pytest.mark.parametrize("nch,sw", [(1, 3), (1, 5), (1, 7), (1, 31), (2, 3), (2, 5), (2, 7), (3, 3), (3, 5), (3, 7)])
def test_fused_window_conv_equals_conv_c_and_conv_sup(nch, sw):
    """The RW -> 2 nf conv over the packed window equals cat(conv_c(x_c), conv_sup(x_sup)) of WindowUnit_l1 (savsr_arch.py:444-458) in
    float64, on windows packed in the kernel's channel order."""
    from savsr_amd.packing import fuse_window_conv, window_record
    nf = 32
    sd = synth.synth_state_dict(synth.manifest_of(_net(dict(num_in_ch=nch, num_feat=nf, num_frame=sw, slid_win=sw, fusion_win=sw)).state_dict()),
                                seed=6)
    T, h, w = sw + 2, 7, 9
    lq = synth.synth_clip(T, nch, h, w, seed=11)[0]
    wins = pack_windows_ref(lq, sw).double()
    assert wins.shape[-1] == window_record(nch, sw) == (16 if nch * sw <= 16 else 32)
    assert not bool(wins[..., nch * sw:].any())
    wt, bt = fuse_window_conv(sd, "p2f_win", nch, sw)
    x = F.pad(lq.double().reshape(1, T * nch, h, w), [0, 1, 0, 1], mode="reflect")[0].reshape(T, nch, h + 1, w + 1)
    g = lambda k: sd[k].double()      # noqa: E731
    for q in range(T - sw + 1):
        it = x[q:q + sw]                                                 # generate_it (:661-668) at centre q + sw // 2
        sup = [i for i in range(sw) if i != sw // 2]
        h_c = F.conv2d(it[sw // 2][None], g("p2f_win.conv_c.weight"), g("p2f_win.conv_c.bias"), padding=1)
        h_s = F.conv2d(it[sup].reshape(1, (sw - 1) * nch, h + 1, w + 1), g("p2f_win.conv_sup.weight"), g("p2f_win.conv_sup.bias"), padding=1)
        got = F.conv2d(wins[q].permute(2, 0, 1)[None], wt.double(), bt.double(), padding=1)
        assert float((got - torch.cat([h_c, h_s], 1)).abs().max()) < 1e-12


def test_shipped_window_conv_fold_is_unchanged():
    """nch = 3, sw = 3: the 16 -> 128 conv over frame t | t-1 | t+1 | zeros, as before."""
    from savsr_amd.packing import fuse_window_conv
    sd = synth.synth_state_dict(seed=2)
    w, b = fuse_window_conv(sd, "f2p_win", 3, 3)
    ref = torch.zeros(128, 16, 3, 3)
    ref[:64, 0:3] = sd["f2p_win.conv_c.weight"].float()
    ref[64:, 3:9] = sd["f2p_win.conv_sup.weight"].float()
    assert torch.equal(w, ref)
    assert torch.equal(b, torch.cat([sd["f2p_win.conv_c.bias"].float(), sd["f2p_win.conv_sup.bias"].float()]))


def tail_float64(p, nch, bias, H, W):
    """The nine shifted taps of P[nch (3 ky + kx) + o] plus the tail bias (what savsr_tail_gather_nch adds before the residual)."""
    pp = F.pad(p[:9 * nch], (1, 1, 1, 1))
    out = bias.double()[:, None, None].repeat(1, H, W)
    for ky in range(3):
        for kx in range(3):
            for o in range(nch):
                out[o] += pp[nch * (3 * ky + kx) + o, ky:ky + H, kx:kx + W]
    return out


@pytest.mark.parametrize("nch,nf,h,w,sc", [(1, 64, 7, 9, (4, 4)), (1, 32, 6, 8, (2.7, 1.6)), (2, 32, 5, 7, (3.5, 2)), (2, 64, 6, 5, (1.5, 3.7))])
def test_nch_row_fold_reproduces_satu_and_tail_conv(nch, nf, h, w, sc):
    """fold_satu_nf with 9 nch live rows of Wt (row p = nch (3 ky + kx) + o, rows 9 nch .. 31 zero), evaluated as the kernels evaluate it,
    equals the oracle's STAUpsample followed by the 3x3 tail conv (nf -> nch) in float64."""
    from savsr_amd.packing import fold_satu_nf, tail_rows27
    sd = synth.synth_state_dict(synth.manifest_of(_net(dict(num_in_ch=nch, num_feat=nf)).state_dict()), seed=4)
    wt = tail_rows27(sd, nf)
    assert float(np.abs(wt[9 * nch:]).max()) == 0.0 and float(np.abs(wt[:9 * nch]).min(axis=1).max()) > 0.0
    m = fold_satu_nf(sd, nf)
    assert float(np.abs(m["fb"][9 * nch:]).max()) == 0.0 and float(np.abs(m["wbe"][..., 9 * nch:]).max()) == 0.0
    x = rnd((1, nf, h, w), 71, 1.0)
    st = rnd((1, nf, h, w), 72, 0.6)
    with torch.no_grad():
        ref = F.conv2d(O.sta_upsample(sd, "upsample", x, sc, st), sd["tail.weight"], sd["tail.bias"], padding=1)[0].double()
    H, W = O.get_hw(h, w, sc)
    p = p32_float64(sd, nf, x, st, sc)
    assert float(p[9 * nch:].abs().max()) == 0.0
    out = tail_float64(p, nch, sd["tail.bias"], H, W)
    err = float((out - ref).abs().max())
    print(nch, nf, sc, "folded float64 vs oracle", err, "magnitude", float(ref.abs().max()))
    assert err <= 1e-5


def test_shipped_tail_rows_are_unchanged():
    """nch = 3: Wt27's rows p = 3 (3 ky + kx) + o, as before."""
    from savsr_amd.packing import tail_rows27
    sd = synth.synth_state_dict(seed=1)
    wt = tail_rows27(sd, 64)
    tw = sd["tail.weight"].double().numpy()
    for ky in range(3):
        for kx in range(3):
            for o in range(3):
                assert np.array_equal(wt[3 * (3 * ky + kx) + o], tw[o, :, ky, kx])
    assert not wt[27:].any()


@pytest.mark.parametrize("kw,reason", [
    (dict(num_in_ch=4), "num_in_ch <= 3"),
    (dict(num_in_ch=6), "9 * num_in_ch rows inside the 32-row MFMA tile"),
    (dict(slid_win=1, num_frame=7), "conv_sup with 0 input channels"),
    (dict(slid_win=4, num_frame=7), "slid_win is odd and >= 3"),
    (dict(slid_win=2, num_frame=7), "slid_win is odd and >= 3"),
    (dict(num_in_ch=2, slid_win=17, num_frame=17, fusion_win=17), "at most 32 channels"),
    (dict(num_frame=7, slid_win=5, fusion_win=5), "WindowUnit_l2.forward raises an IndexError"),
])
def test_refusals_name_their_reason(kw, reason):
    from savsr_amd.engine import HipEngine
    msg = HipEngine.window_limit(_cfg(**kw))
    assert msg is not None and reason in msg, msg


@pytest.mark.parametrize("kw", [dict(num_in_ch=1), dict(num_in_ch=2), dict(num_in_ch=3), dict(num_in_ch=1, slid_win=31, num_frame=31, fusion_win=31),
                                dict(num_in_ch=2, slid_win=15, num_frame=15, fusion_win=15), dict(num_frame=5, slid_win=5),
                                dict(num_frame=7, slid_win=7, fusion_win=7), dict(num_in_ch=1, num_frame=9, interval=1),
                                dict(num_frame=9, interval=1, slid_win=5), dict(num_frame=9, interval=1, fusion_win=3)])
def test_supported_windows_pass(kw):
    from savsr_amd.engine import HipEngine
    assert HipEngine.window_limit(_cfg(**kw)) is None


def test_tail_fold_refuses_four_channels():
    from savsr_amd.packing import tail_rows27
    sd = synth.synth_state_dict(synth.manifest_of(_net(dict(num_in_ch=4, num_feat=32)).state_dict()), seed=0)
    with pytest.raises(ValueError, match="num_in_ch <= 3"):
        tail_rows27(sd, 32)
