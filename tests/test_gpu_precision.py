"""The precision mode "fp16" on the GPU (SAVSR.set_precision): the fp16-operand conv kernels against float64 convolutions of fp16-rounded
operands, the OSConv fp16 images, the whole network against the CPU emulation's drift (tools/gen_golden_precision.py), the bitwise
properties of DESIGN.md section 3 within the mode, switching modes, and the CLIs."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from savsr_amd.utils import synth
from tests.golden_cases import OSCONV_CASES, OSCONV_SCALES, rnd
from tests.precision_cases import CLIP_SEED, GT_CASE, PRECISION_CASES, WEIGHT_SEED, psnr_y, synth_gt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
KBOUND = 2e-6          # per-kernel bound: max-abs error / max over the tensor of sum |x w| (accumulation order only)


@pytest.fixture(scope="module")
def eng(synth_sd):
    from savsr_amd.engine import HipEngine
    from savsr_amd.archs.savsr_arch import SAVSR
    return HipEngine(synth_sd, SAVSR().cfg, DEV)


@pytest.fixture(scope="module")
def pgold():
    return np.load(os.path.join(ROOT, "tests", "golden", "precision_outputs.npz"))


def _net(kw=None, seed=WEIGHT_SEED):
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR(**(kw or {})).eval()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=seed), strict=True)
    return net.to(DEV)


def cl(x):
    return x.permute(1, 2, 0).contiguous().to(DEV)


def pl(t):
    return t.detach().cpu().permute(2, 0, 1).contiguous()


def f16(t):
    return t.to(torch.float32).to(torch.float16).to(torch.float64)


def _run_conv(eng, precision, x, wimg, bias, cout, cin, ks, nsrc, algo, epi):
    """One conv launch through the engine's launcher in `precision`; returns the planar output [cout, h, w] (CPU, fp32)."""
    from savsr_amd import engine as E
    from savsr_amd._lib import ACT_LRELU
    _, h, w = x.shape
    sch = cin // nsrc
    xall = cl(x)
    srcs = [eng.full(xall, sch, i * sch) for i in range(nsrc)]
    weights = (wimg.to(DEV), bias.to(DEV), cout, cin, ks) + ((algo,) if algo is not None else ())
    o = torch.full((h, w, cout), float("nan"), device=DEV)
    kw = dict(res1=eng.full(cl(epi["res"])))
    if "mul" in epi:
        kw.update(mul_px=epi["mul"].to(DEV), res2=eng.full(cl(epi["res2"])), res2_scale=0.9)
    if "pool" in epi:
        kw["pool"] = (epi["pool"], 0, cout)
    old = eng.precision
    eng.precision = precision
    try:
        eng.conv("test", srcs, E.Src(o, cout, cout), h, w, ACT_LRELU, 0.2, weights=weights, **kw)
        torch.cuda.synchronize()
    finally:
        eng.precision = old
    return pl(o)


def _epilogue(acc, bias, epi):
    y = F.leaky_relu(acc + bias.double().view(-1, 1, 1), 0.2)
    if "mul" in epi:
        y = y * epi["mul"].double()
    y = y + epi["res"].double()
    if "mul" in epi:
        y = y + 0.9 * epi["res2"].double()
    return y


def _case(cin, cout, ks, h, w, seed, generic):
    g = np.random.RandomState(seed)
    wt = torch.from_numpy((g.standard_normal((cout, cin, ks, ks)) / np.sqrt(cin * ks * ks)).astype(np.float32))
    bias = torch.from_numpy(g.standard_normal(cout).astype(np.float32))
    x = torch.from_numpy(g.standard_normal((cin, h, w)).astype(np.float32))
    epi = dict(res=torch.from_numpy(g.standard_normal((cout, h, w)).astype(np.float32)))
    if generic:
        epi["mul"] = torch.from_numpy(g.uniform(0, 1, (h, w)).astype(np.float32))
        epi["res2"] = torch.from_numpy(g.standard_normal((cout, h, w)).astype(np.float32))
    return wt, bias, x, epi


# (ksize, nsrc, src_ch, cout, h, w, generic epilogue, throughput tiling): 8-row tiles, 16-row tiles (the throughput algo from 100 tiles),
# 1x1, cout < 64, multi-source
DIRECT = [(3, 1, 64, 64, 10, 12, False, False), (3, 3, 64, 64, 9, 40, True, False), (3, 2, 64, 64, 40, 70, False, False),
          (3, 5, 64, 128, 8, 35, False, False), (1, 3, 64, 64, 7, 50, False, False), (1, 2, 64, 64, 40, 70, True, False),
          (3, 1, 16, 16, 5, 6, False, False), (3, 1, 16, 1, 10, 12, True, False), (3, 1, 64, 32, 13, 31, False, False),
          (3, 1, 64, 64, 180, 320, False, True), (1, 2, 64, 64, 180, 320, True, True)]


@pytest.mark.parametrize("ks,nsrc,sch,cout,h,w,generic,tp", DIRECT)
def test_conv_f16_direct(eng, ks, nsrc, sch, cout, h, w, generic, tp):
    """savsr_conv2d_batch_f16, direct form: a float64 conv of the fp16-rounded operands within 2e-6 of max sum |x w|; the split path
    (savsr_conv2d_batch) on the same inputs is NOT within that bound of the fp16 emulation (its products are not fp16-rounded)."""
    from savsr_amd import _lib
    from savsr_amd.packing import pack_conv_weight, pack_conv_weight_f16
    cin = nsrc * sch
    wt, bias, x, epi = _case(cin, cout, ks, h, w, cin * 7 + cout + h + ks, generic)
    acc = F.conv2d(f16(x)[None], f16(wt), None, padding=ks // 2)[0]
    mag = float(F.conv2d(f16(x).abs()[None], f16(wt).abs(), None, padding=ks // 2)[0].max())
    ref = _epilogue(acc, bias, epi)
    algo = _lib.CONV_DIRECT_THROUGHPUT if tp else None
    got = _run_conv(eng, "fp16", x, pack_conv_weight_f16(wt), bias, cout, cin, ks, nsrc, algo, epi)
    split = _run_conv(eng, "fp32", x, pack_conv_weight(wt), bias, cout, cin, ks, nsrc, algo, epi)
    e16 = float((got.double() - ref).abs().max()) / mag
    e32 = float((split.double() - ref).abs().max()) / mag
    print(f"direct ks{ks} {nsrc}x{sch}->{cout} {h}x{w}: fp16 {e16:.2e}  split {e32:.2e} of max sum|xw| {mag:.1f}")
    assert e16 < KBOUND
    assert e32 > KBOUND


def _wy_reference(x, wt):
    """float64 F(2,3) along y on fp32-transformed, fp16-rounded V and U (conv_wy.hip's arithmetic with exact products)."""
    from savsr_amd.packing import wy_transform_f64
    cin, h, w = x.shape
    npair = (h + 1) // 2
    xp = torch.zeros(cin, 2 * npair + 2, w)
    xp[:, 1:h + 1] = x
    d = [xp[:, i:i + 2 * npair:2] for i in range(4)]              # rows Y-1 .. Y+2 of every pair: [cin, npair, w] each, fp32
    v = [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]      # fp32 arithmetic, as the staging
    u16 = torch.from_numpy(wy_transform_f64(wt).astype(np.float16).astype(np.float64))      # [4][cout][cin][3]: float64 U rounded ONCE
    m, a = [], []
    for i in range(4):
        ui = u16[i].unsqueeze(2)                                    # [cout][cin][1][3]
        m.append(F.conv2d(f16(v[i])[None], ui, None, padding=(0, 1))[0])
        a.append(F.conv2d(f16(v[i]).abs()[None], ui.abs(), None, padding=(0, 1))[0])
    out = torch.stack([m[0] + m[1] + m[2], m[1] - m[2] - m[3]], 2).reshape(wt.shape[0], 2 * npair, w)[:, :h]
    mag = torch.stack([a[0] + a[1] + a[2], a[1] + a[2] + a[3]], 2).reshape(wt.shape[0], 2 * npair, w)[:, :h]
    return out, float(mag.max())


# (nsrc, src_ch, cout, h, w, generic): strip-tile heights (h % 16 = 2, 4, 8), multi-source, 128 channels, the generic epilogue
WY = [(1, 64, 64, 18, 40, False), (3, 64, 64, 36, 70, True), (2, 64, 64, 20, 33, False), (5, 64, 128, 24, 35, False),
      (1, 64, 64, 23, 100, True), (1, 16, 64, 17, 30, False)]


@pytest.mark.parametrize("nsrc,sch,cout,h,w,generic", WY)
def test_conv_f16_winograd_y(eng, nsrc, sch, cout, h, w, generic):
    """savsr_conv2d_batch_f16, Winograd-y form (WINOGRAD_Y and _THROUGHPUT: same bits), against the float64 F(2,3) emulation; the
    split path misses the bound."""
    from savsr_amd import _lib
    from savsr_amd.packing import pack_conv_weight_wy, pack_conv_weight_wy_f16
    cin = nsrc * sch
    wt, bias, x, epi = _case(cin, cout, 3, h, w, cin * 5 + cout + h, generic)
    acc, mag = _wy_reference(x, wt)
    ref = _epilogue(acc, bias, epi)
    img = pack_conv_weight_wy_f16(wt)
    got = _run_conv(eng, "fp16", x, img, bias, cout, cin, 3, nsrc, _lib.CONV_WINOGRAD_Y, epi)
    got_tp = _run_conv(eng, "fp16", x, img, bias, cout, cin, 3, nsrc, _lib.CONV_WINOGRAD_Y_THROUGHPUT, epi)
    split = _run_conv(eng, "fp32", x, pack_conv_weight_wy(wt), bias, cout, cin, 3, nsrc, _lib.CONV_WINOGRAD_Y, epi)
    assert torch.equal(got, got_tp)
    e16 = float((got.double() - ref).abs().max()) / mag
    e32 = float((split.double() - ref).abs().max()) / mag
    print(f"winograd-y {nsrc}x{sch}->{cout} {h}x{w}: fp16 {e16:.2e}  split {e32:.2e} of max sum|UV| {mag:.1f}")
    assert e16 < KBOUND
    assert e32 > KBOUND


def test_conv_f16_pool_epilogue(eng):
    """Fused pooling partials in the fp16 form: their per-channel total is the sum of the stored outputs."""
    from savsr_amd import _lib
    from savsr_amd.packing import pack_conv_weight_f16, pack_conv_weight_wy_f16
    h, w, cin, cout = 30, 70, 64, 64
    wt, bias, x, epi = _case(cin, cout, 3, h, w, 99, False)
    for img, algo in ((pack_conv_weight_f16(wt), None), (pack_conv_weight_wy_f16(wt), _lib.CONV_WINOGRAD_Y)):
        rows = eng.pool_rows(h, w)
        pool = torch.zeros(rows * cout, device=DEV)
        e = dict(epi, pool=pool)
        out = _run_conv(eng, "fp16", x, img, bias, cout, cin, 3, 1, algo, e)
        tot = pool.view(rows, cout).double().sum(0).cpu()
        assert torch.allclose(tot, out.double().sum((1, 2)), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("tag,pfx,cin", OSCONV_CASES)
@pytest.mark.parametrize("sc", OSCONV_SCALES)
def test_osconv_f16_images(eng, synth_sd, tag, pfx, cin, sc):
    """savsr_osconv_weights_batch_f16: the direct and the Winograd-y fp16 images are float64 W'' (from the launch's own gates) rounded to
    fp16, within 1 fp16 ulp; unaddressed entries stay zero."""
    from savsr_amd.packing import conv_pack_index, conv_wy_pack_index, wy_transform_f64
    h, w = 10, 12
    x = rnd((1, cin, h, w), 11 + cin, 0.7)
    xall = cl(x[0])
    nsrc = cin // 64
    srcs = [eng.full(xall, 64, i * 64) for i in range(nsrc)]
    ent = eng.osc[pfx]
    cout, knum = ent["cout"], ent["knum"]
    bank = synth_sd[pfx + ".weight"].double()                          # [K, cout, cin, 3, 3]
    for wy in (False, True) if cout % 64 == 0 else (False,):
        ent["wdyn"].fill_(0), ent["wdyn_wy"].fill_(0)
        eng.precision = "fp16"
        try:
            eng.osconv_weights(pfx, srcs, h, w, sc, wy=wy)
        finally:
            eng.precision = "fp32"
        torch.cuda.synchronize()
        att = ent["att"].double().cpu()
        ca, fa, sa, ka = att[:cin], att[cin:cin + cout], att[cin + cout:cin + cout + 9], att[cin + cout + 9:]
        wpp = (fa.view(-1, 1, 1, 1) * ca.view(1, -1, 1, 1) * sa.view(1, 1, 3, 3) * (ka.view(-1, 1, 1, 1, 1) * bank).sum(0))
        if wy:
            idx, total = conv_wy_pack_index(cout, cin)
            ref = torch.from_numpy(wy_transform_f64(wpp.float())).reshape(-1)
            img = ent["wdyn_wy"]
        else:
            idx, total = conv_pack_index(cout, cin, 3)
            ref = wpp.reshape(-1)
            img = ent["wdyn"]
        got = img.view(torch.float16)[:total].cpu()
        vals = got[torch.from_numpy(idx)].double()
        ulp = torch.from_numpy(np.spacing(np.abs(ref.numpy()).astype(np.float16)).astype(np.float64))
        d = (vals - ref).abs() / ulp
        print(tag, sc, "wy" if wy else "direct", "max ulp", float(d.max()))
        assert float(d.max()) <= 1.0
        mask = torch.ones(total, dtype=torch.bool)
        mask[torch.from_numpy(idx)] = False
        assert not bool(got[mask].abs().max() > 0) if bool(mask.any()) else True


def _run_net(net, name, kw, h, w, sc):
    lq = synth.synth_clip(7, net.cfg["num_in_ch"], h, w, seed=CLIP_SEED).to(DEV)
    net.set_scale(sc)
    return net(lq)[0].cpu().numpy()


@pytest.mark.parametrize("name,kw,h,w,sc", PRECISION_CASES)
def test_network_f16_drift(pgold, name, kw, h, w, sc):
    """fp16 mode at the golden cases: max-abs <= 3x and mean-abs <= 2x the CPU emulation's drift against the fp32 output;
    |dPSNR-Y| <= 0.01 dB on the GT case."""
    net = _net(kw)
    net.set_precision("fp16")
    out = _run_net(net, name, kw, h, w, sc)
    ref = pgold[f"{name}/fp32"]
    d = np.abs(out.astype(np.float64) - ref)
    emax, emean = (float(v) for v in pgold[f"{name}/drift"])
    print(f"{name}: GPU fp16 max-abs {d.max():.3e} ({d.max() / emax:.2f}x emulated), mean-abs {d.mean():.3e} ({d.mean() / emean:.2f}x)")
    assert d.max() <= 3 * emax and d.mean() <= 2 * emean
    assert d.max() > 0                                         # the mode is in effect
    if name == GT_CASE:
        gt = synth_gt(ref)
        dp = psnr_y(out, gt) - float(pgold["gt/psnr_fp32"])
        print(f"  dPSNR-Y {dp:+.6f} dB (emulated {float(pgold['gt/psnr_fp16emu']) - float(pgold['gt/psnr_fp32']):+.6f})")
        assert abs(dp) <= 0.01


@pytest.fixture(scope="module")
def net_f16():
    net = _net()
    net.set_precision("fp16")
    return net


def test_f16_eager_captured_replayed_equal(net_f16):
    """Within fp16 mode: the eager launch sequence, the captured graphs' first run and a replay give the same bits."""
    eng = net_f16.engine()
    lq = synth.synth_clip(7, 3, 20, 34, seed=3).to(DEV)
    sc = (2.5, 3.0)
    H, W = round(20 * sc[0]), round(34 * sc[1])
    eager = torch.empty(3, H, W, device=DEV)
    eng.forward_one(lq[0], sc, eager)
    net_f16.set_scale(sc)
    a = net_f16(lq)[0]
    b = net_f16(lq)[0]
    torch.cuda.synchronize()
    assert torch.equal(eager, a) and torch.equal(a, b)


def test_f16_forward_many_grouping(net_f16):
    """forward_many with 1, 2 and 4 clips equals the clips run alone, bit for bit, in fp16 mode."""
    clips = [synth.synth_clip(7, 3, 16, 24, seed=20 + i)[0].to(DEV) for i in range(4)]
    sc = (3.0, 3.0)
    alone = [net_f16.forward_many([c], [sc])[0] for c in clips]
    for n in (1, 2, 4):
        outs = net_f16.forward_many(clips[:n], [sc] * n)
        for i in range(n):
            assert torch.equal(outs[i], alone[i]), (n, i)


def test_f16_upscale_video_equals_forward_many(net_f16):
    from savsr_amd.harness import window_indices
    n, h, w = 8, 12, 14
    frames = torch.from_numpy(np.random.RandomState(4).uniform(0, 1, (n, 3, h, w)).astype(np.float32)).to(DEV)
    sc = (2.0, 2.0)
    out = net_f16.upscale_video(frames, scale=sc)
    wins = [window_indices(i, n, net_f16.num_frame, "reflection") for i in range(n)]
    ref = net_f16.forward_many([frames[wi] for wi in wins], [sc] * n)
    for i in range(n):
        assert torch.equal(out[i], ref[i]), i


def test_mode_switching():
    """Alternating fp32 and fp16 on one (shape, scale): each mode reproduces its own first output bit for bit, and fp32 after fp16 use
    equals a fresh net that never used fp16."""
    lq = synth.synth_clip(7, 3, 18, 22, seed=9).to(DEV)
    fresh = _net()
    fresh.set_scale((2.0, 3.0))
    ref32 = fresh(lq)
    net = _net()
    net.set_scale((2.0, 3.0))
    first = {}
    for mode in ("fp32", "fp16", "fp32", "fp16", "fp32"):
        net.set_precision(mode)
        o = net(lq)
        if mode in first:
            assert torch.equal(o, first[mode]), mode
        first.setdefault(mode, o)
    assert torch.equal(first["fp32"], ref32)
    assert not torch.equal(first["fp16"], first["fp32"])
    many32 = net.forward_many([lq[0]], [(2.0, 3.0)])[0]
    assert torch.equal(many32, fresh.forward_many([lq[0]], [(2.0, 3.0)])[0])


def test_f16_precision_survives_to_and_load_state_dict():
    net = _net()
    net.set_precision("fp16")
    net.load_state_dict(net.state_dict())
    net = net.to(DEV)
    assert net.precision == "fp16" and net.engine().precision == "fp16"


def test_cli_upscale_precision_f16(tmp_path):
    from PIL import Image
    from savsr_amd import io as sio
    from savsr_amd.upscale import main
    net = _net()
    n, h, w = 8, 12, 14
    u8 = np.random.RandomState(13).randint(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    src, dst = tmp_path / "lr", tmp_path / "sr"
    src.mkdir()
    names = [f"im{i:03d}.png" for i in range(n)]
    for i, nm in enumerate(names):
        Image.fromarray(u8[i]).save(src / nm)
    ckpt = tmp_path / "net.pth"
    sio.save_network(net, str(ckpt))
    assert main(["-i", str(src), "-o", str(dst), "--scale", "2", "--checkpoint", str(ckpt), "--chunk", "4", "--precision", "fp16"]) == 0
    net.set_precision("fp16")
    ref = net.upscale_video(torch.from_numpy(u8), scale=(2, 2), out="uint8").cpu().numpy()
    for i, nm in enumerate(names):
        assert np.array_equal(np.asarray(Image.open(dst / nm)), ref[i]), nm
