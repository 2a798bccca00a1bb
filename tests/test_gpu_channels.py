"""num_in_ch / slid_win checkpoints beside the shipped 3 / 3 on the GPU: the generic window packing (savsr_pack_windows_nch), the
plane-count HR entry (savsr_satu_nf_hr_planes) and the nch tail gather (savsr_tail_gather_nch) against torch / float64 references, and
whole networks against the REFERENCE's golden outputs (tests/golden/channels_outputs.npz), the CPU oracle, the batched flow and the
YAML surface."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import savsr_oracle as O
from savsr_amd.utils import synth
from tests.channel_cases import CHANNEL_CASES
from tests.golden_cases import rnd
from tests.test_channels import pack_windows_ref, tail_float64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def _sd(cfg, seed=3):
    from savsr_amd.archs.savsr_arch import SAVSR
    return synth.synth_state_dict(synth.manifest_of(SAVSR(**cfg).state_dict()), seed=seed)


def _engine(sd, cfg):
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.engine import HipEngine
    return HipEngine(sd, SAVSR(**cfg).cfg, DEV)


def _net(sd, cfg):
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR(**cfg)
    net.load_state_dict(sd, strict=True)
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def sd_c1():
    return _sd(dict(num_in_ch=1))


def _lib():
    from savsr_amd import _lib as L
    return L.load()


@pytest.mark.parametrize("nch,sw", [(1, 3), (1, 5), (1, 7), (2, 3), (2, 5), (2, 7), (3, 3), (3, 5), (3, 7), (1, 31)])
@pytest.mark.parametrize("h,w", [(7, 9), (8, 5)])
def test_pack_windows_nch_bitwise(nch, sw, h, w):
    from savsr_amd.packing import window_record
    lib = _lib()
    T = sw + 2
    lq = synth.synth_clip(T, nch, h, w, seed=nch * 10 + sw)[0]
    ref = pack_windows_ref(lq, sw)
    rw = window_record(nch, sw)
    hp, wp = h + (h & 1), w + (w & 1)
    n = (T - sw + 1) * hp * wp * rw
    out = torch.full((n + 64,), float("nan"), device=DEV)          # poisoned: every float of the windows is written, nothing beyond
    lqd = lq.contiguous().to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.savsr_pack_windows_nch(lqd.data_ptr(), out.data_ptr(), T, nch, sw, h, w, hp, wp, st) == 0
    torch.cuda.synchronize()
    got = out[:n].cpu().reshape(ref.shape)
    assert torch.equal(got, ref)
    assert bool(torch.isnan(out[n:]).all())
    if nch == 3 and sw == 3:                                         # the shipped kernel's windows, bit for bit
        old = torch.full((n,), float("nan"), device=DEV)
        assert lib.savsr_pack_windows(lqd.data_ptr(), old.data_ptr(), T, h, w, hp, wp, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(old.cpu(), out[:n].cpu())


def test_pack_windows_nch_refuses_bad_windows():
    lib = _lib()
    buf = torch.zeros(4096, device=DEV)
    for nch, sw in ((1, 1), (1, 4), (3, 11), (0, 3)):
        assert lib.savsr_pack_windows_nch(buf.data_ptr(), buf.data_ptr(), 12, nch, sw, 4, 4, 4, 4, 0) < 0


@pytest.mark.parametrize("nch,nf", [(1, 64), (2, 32), (1, 32), (2, 64)])
def test_hr_planes_equal_the_27_plane_call(nch, nf):
    """savsr_satu_nf_hr_planes(planes = 9 nch) writes the first 9 nch planes of savsr_satu_nf_hr bit for bit, and nothing else."""
    e = _engine(_sd(dict(num_in_ch=nch, num_feat=nf)), dict(num_in_ch=nch, num_feat=nf))
    assert e.satu_generic and e.tail_planes == 9 * nch
    for (h, w, sc) in [(13, 17, (2.7, 3.3)), (19, 23, (3.9, 3.9)), (6, 5, (2.95, 3.75))]:
        H, W = O.get_hw(h, w, sc)
        pad = 20
        e._select((7, nch, h, w), sc)
        x = rnd((1, nf, h, w), 61, 1.0)
        st = rnd((1, nf, h, w), 62, 0.6)
        xd, sd_ = (t[0].permute(1, 2, 0).contiguous().to(DEV) for t in (x, st))
        lrcat = e.satu_nf_lr(e.full(xd), e.full(sd_), w, h, w)
        p27 = torch.full((27, H * W + pad), float("nan"), device=DEV)
        pn = torch.full((27, H * W + pad), float("nan"), device=DEV)
        e.tail_planes = 27
        e.satu_nf_hr(lrcat, h, w, sc, p27, H * W + pad)
        e.tail_planes = 9 * nch
        e.satu_nf_hr(lrcat, h, w, sc, pn, H * W + pad)
        torch.cuda.synchronize()
        k = 9 * nch
        assert torch.equal(pn[:k, :H * W].cpu(), p27[:k, :H * W].cpu())
        assert bool(torch.isfinite(pn[:k, :H * W]).all())
        assert bool(torch.isnan(pn[:k, H * W:]).all()) and bool(torch.isnan(pn[k:]).all()), "nothing beyond the live planes is written"
        assert float(p27[k:, :H * W].abs().max()) == 0.0                   # (Wt rows 9 nch .. 26 are zero)


@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("h,w,sc", [(7, 9, (4, 4)), (6, 5, (2.95, 3.75)), (13, 17, (2.7, 3.3))])
def test_tail_gather_nch_vs_float64(nch, h, w, sc):
    lib = _lib()
    H, W = O.get_hw(h, w, sc)
    pad = 12
    p = rnd((9 * nch, H, W), 91 + nch, 1.0)
    bias = rnd((nch,), 92, 0.5)
    center = torch.rand(nch, h, w, generator=torch.Generator().manual_seed(93))
    pd = torch.full((9 * nch, H * W + pad), float("nan"), device=DEV)
    pd[:, :H * W] = p.reshape(9 * nch, -1).to(DEV)
    bd, cd = bias.to(DEV), center.contiguous().to(DEV)
    out = torch.full((nch * H * W + 16,), float("nan"), device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.savsr_tail_gather_nch(pd.data_ptr(), H * W + pad, nch, bd.data_ptr(), cd.data_ptr(), h, w, H, W, out.data_ptr(), st) == 0
    torch.cuda.synchronize()
    got = out[:nch * H * W].cpu().reshape(nch, H, W).double()
    assert bool(torch.isnan(out[nch * H * W:]).all())
    ref = tail_float64(p.double(), nch, bias, H, W) + F.interpolate(center[None].double(), size=(H, W), mode="bilinear", align_corners=False)[0]
    err = float((got - ref).abs().max())
    print(nch, (h, w, sc), "tail gather max-abs vs float64", err)
    assert err < 1e-5
    if nch == 3:                                                        # the shipped 27-plane tail, to rounding
        o27 = torch.full((3 * H * W,), float("nan"), device=DEV)
        assert lib.savsr_tail_gather(pd.data_ptr(), H * W + pad, bd.data_ptr(), cd.data_ptr(), h, w, H, W, o27.data_ptr(), st) == 0
        torch.cuda.synchronize()
        assert float((o27.cpu() - out[:3 * H * W].cpu()).abs().max()) < 2e-6


@pytest.mark.parametrize("name,cfg,h,w,sc", CHANNEL_CASES)
def test_network_vs_reference_golden(name, cfg, h, w, sc):
    """End to end: within 5e-5 max-abs of the reference's output; eager, captured and replayed runs bitwise equal."""
    gold = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "channels_outputs.npz"))[f"{name}/sr"])
    net = _net(_sd(cfg), cfg)
    net.set_scale(sc)
    nch = cfg.get("num_in_ch", 3)
    lq = synth.synth_clip(cfg.get("num_frame", 7), nch, h, w, seed=5).to(DEV)
    taps = {}
    eager = net(lq, taps=taps).cpu()                     # taps force the eager launch sequence
    a = net(lq).cpu()                                    # captured
    b = net(lq).cpu()                                    # replayed
    assert tuple(taps["p27"].shape[0:1]) == (9 * nch,)
    assert a.shape == gold.shape
    err = float((a - gold).abs().max())
    print(name, "max-abs vs reference", err)
    assert err < 5e-5
    assert torch.equal(a, b) and torch.equal(a, eager)


def test_network_64x96_x4_vs_oracle(sd_c1):
    cfg = dict(num_in_ch=1)
    net = _net(sd_c1, cfg)
    net.set_scale((4, 4))
    lq = synth.synth_clip(7, 1, 64, 96, seed=9)
    out = net(lq.to(DEV)).cpu()
    with torch.no_grad():
        ref = O.forward(sd_c1, lq, (4, 4), cfg=cfg)
    assert out.shape == ref.shape == (1, 1, 256, 384)
    err = float((out - ref).abs().max())
    print("nch 1: 64x96 x4 max-abs vs oracle", err)
    assert err < 5e-5


def test_forward_many_group_equals_one_clip_runs(sd_c1):
    """nch = 1, nf = 64: clips of one (shape, scale) batched into one launch sequence equal their own runs bit for bit."""
    cfg = dict(num_in_ch=1)
    net = _net(sd_c1, cfg)
    clips = [synth.synth_clip(7, 1, 20, 24, seed=s)[0].to(DEV) for s in (1, 2, 3)]
    sc = (2.5, 3.5)
    group = net.forward_many(clips, [sc] * 3)
    for c, g in zip(clips, group):
        assert g.shape == (1,) + O.get_hw(20, 24, sc)
        one = net.forward_many([c], [sc])[0]
        assert torch.equal(g, one)
    with torch.no_grad():
        ref = O.forward(sd_c1, clips[1].cpu().unsqueeze(0), sc, cfg=cfg)[0]
    assert float((group[1].cpu() - ref).abs().max()) < 5e-5


def test_batched_forward_routes_nch(sd_c1):
    """A batch of b = 3 clips through SAVSR.forward (several streams, batched launch sequences) equals the oracle per clip."""
    cfg = dict(num_in_ch=1)
    net = _net(sd_c1, cfg)
    net.set_scale((2, 3))
    lq = synth.synth_clip(7, 1, 16, 18, seed=4, batch=3)
    out = net(lq.to(DEV)).cpu()
    with torch.no_grad():
        ref = O.forward(sd_c1, lq, (2, 3), cfg=cfg)
    assert out.shape == ref.shape and float((out - ref).abs().max()) < 5e-5


def test_four_channels_are_refused_at_engine_build():
    cfg = dict(num_in_ch=4, num_feat=32)
    net = _net(_sd(cfg, seed=0), cfg)
    net.set_scale((2, 2))
    with pytest.raises(RuntimeError, match=r"num_in_ch <= 3"):
        net(synth.synth_clip(7, 4, 8, 8, seed=0).to(DEV))


def test_run_test_refuses_one_channel(tmp_path):
    from savsr_amd import io as sio
    from savsr_amd import metrics as M
    from savsr_amd.options import parse_test_options
    from savsr_amd.test import run_test
    from tests.test_gpu_run_test import YAML
    root = str(tmp_path)
    for i in range(5):
        sio.imwrite(M.tensor2img(synth.synth_gt(3, 45, 62, seed=40 + i)), os.path.join(root, "GT", "city", f"{i:08d}.png"))
    text = YAML.format(root=root).replace("num_in_ch: 3", "num_in_ch: 1")
    assert "num_in_ch: 1" in text
    with pytest.raises(NotImplementedError, match=r"3-channel .*1-channel metrics are not supported"):
        run_test(parse_test_options(text, root_path=root))
