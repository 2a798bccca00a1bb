"""The folded RCAB on the GPU (savsr_rcab_gate_weights_batch, engine.rcab with SAVSR_RCAB_FOLD): the gate from conv.0's
output against a float64 gate of conv.2's output, the generated image and bias bit for bit, one whole RCAB against float64 with the fold
on and off, independence of the clip grouping and the stream, and stale LDS contents."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from savsr_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PFX = "RG.1.residual_group.2.rcab"


def _engine(nf):
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.engine import HipEngine
    sd = synth.synth_state_dict(synth.manifest_of(SAVSR(num_feat=nf).state_dict()), seed=3) if nf != 64 else synth.synth_state_dict(seed=0)
    return sd, HipEngine(sd, SAVSR(num_feat=nf).cfg, DEV)


@pytest.fixture(scope="module")
def e64():
    return _engine(64)


@pytest.fixture(scope="module")
def e32():
    return _engine(32)


def _which(nf, e64, e32):
    return e64 if nf == 64 else e32


def cl(x):
    return x.permute(1, 2, 0).contiguous().to(DEV)


def _r1_and_partials(eng, nf, h, w, seed):
    """r1 = a ReLU output [nf][h][w] (fp32, CPU), its channel-last device copy and pool partials as conv.0 writes them: one row per
    8-row x 32-column tile, any summation inside a tile (here torch's)."""
    g = torch.Generator().manual_seed(seed)
    r1 = torch.relu(torch.randn(nf, h, w, generator=g))
    rows = []
    for y in range(0, h, 8):
        for x in range(0, w, 32):
            rows.append(r1[:, y:y + 8, x:x + 32].sum((1, 2)))
    part = torch.stack(rows).contiguous()
    assert part.shape[0] == eng.pool_rows(h, w)
    return r1, cl(r1), part.to(DEV)


def _gate64(sd, r1):
    """float64 gate of savsr_arch.py:514-520 on conv.2's output."""
    d = lambda k: sd[PFX + k].double()
    r2 = F.conv2d(r1.double()[None], d(".2.weight"), d(".2.bias"), padding=1)[0]
    cm = sd[PFX + ".3.attention.1.weight"].shape[0]
    z = torch.relu(d(".3.attention.1.weight").reshape(cm, -1) @ r2.mean((1, 2)) + d(".3.attention.1.bias"))
    return torch.sigmoid(d(".3.attention.3.weight").reshape(-1, cm) @ z + d(".3.attention.3.bias")), r2


def _launch(eng, r1d, part, h, w, wy):
    eng.nb = 1
    wd = eng.rcab_gate_weights(PFX, eng.full(r1d), part, h, w, wy=wy)
    torch.cuda.synchronize()
    return wd


@pytest.mark.parametrize("nf", [64, 32])
@pytest.mark.parametrize("h,w", [(180, 320), (2, 2), (2, 40), (17, 33), (36, 70), (64, 600)])
def test_gate_vs_float64(e64, e32, nf, h, w):
    """(a) g from the kernel (fp32 sums of conv.0's output, border form) against the float64 gate of conv.2's output: <= 1e-6.
    Measured on MI355X: 3.8e-8 ... 5.6e-8 over these twelve cases (180x320: 4.6e-8 at 64 channels, 4.8e-8 at 32)."""
    sd, eng = _which(nf, e64, e32)
    r1, r1d, part = _r1_and_partials(eng, nf, h, w, seed=h + w)
    eng.rcab_scr["gate"].fill_(float("nan"))
    _launch(eng, r1d, part, h, w, False)
    ref, _ = _gate64(sd, r1)
    err = float((eng.rcab_scr["gate"].cpu().double() - ref).abs().max())
    print(f"nf {nf} {h}x{w}: gate max-abs vs float64 {err:.3e}")
    assert err <= 1e-6


def _restate(eng, master, f16):
    """split(g * master) in torch from the kernel's own g: unit u = 64 group + lane holds 8 elements of output channel
    cob * cot + 32 t + (lane & 31)."""
    nf = eng.nf
    g = eng.rcab_scr["gate"].clone()
    cot = 64 if nf > 32 else 32
    nt = cot // 32
    units = master.numel() // 8
    grp = torch.arange(units, device=DEV) // 64
    ln = torch.arange(units, device=DEV) % 64
    per_cob = units // 64 // max(1, nf // cot)
    co = (grp // per_cob) * cot + 32 * (grp % nt) + (ln & 31)
    x = (g[co][:, None] * master.view(units, 8))                         # one fp32 product per element
    if f16:
        return x.to(torch.float16).view(torch.int16).reshape(-1)
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    img = torch.stack([hi.view(-1, 64, 8), lo.view(-1, 64, 8)], 1)       # [group][part][lane][8]
    return img.contiguous().view(torch.int16).reshape(-1)


@pytest.mark.parametrize("nf,wy", [(64, False), (64, True), (32, False)])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_image_and_bias_bit_for_bit(e64, e32, nf, wy, precision):
    """(b) the image and the bias equal a torch restatement of split(g master) / g b bit for bit: both forms, both precision modes,
    num_feat 64 and 32 (cout 32: direct form only)."""
    sd, eng = _which(nf, e64, e32)
    h, w = 20, 45
    r1, r1d, part = _r1_and_partials(eng, nf, h, w, seed=5)
    ent, scr = eng.rcab_w[PFX], eng.rcab_scr
    eng.set_precision(precision)
    try:
        scr["wimg"].fill_(0x7FC0)
        wd = _launch(eng, r1d, part, h, w, wy)
    finally:
        eng.set_precision("fp32")
    master = ent["master_wy"] if wy else ent["master"]
    ref = _restate(eng, master, precision == "fp16")
    got = scr["wimg"][:ref.numel()]
    assert torch.equal(got, ref)
    assert bool((scr["wimg"][ref.numel():] == 0x7FC0).all())             # nothing beyond the image is written
    assert torch.equal(scr["bias"], scr["gate"] * ent["bias"])
    assert wd[0] is scr["wimg"] and wd[1] is scr["bias"] and (len(wd) == 6) == wy
    if precision == "fp32":      # the master is what the static image splits, in the same order
        from savsr_amd.packing import split_bf16_image
        static = eng.pw_wy[PFX + ".2"] if wy else eng.pw[PFX + ".2"][0]
        assert torch.equal(static, split_bf16_image(master))


def _rcab64(sd, x):
    d = lambda k: sd[PFX + k].double()
    r1 = torch.relu(F.conv2d(x.double()[None], d(".0.weight"), d(".0.bias"), padding=1))[0]
    g, r2 = _gate64(sd, r1)
    return x.double() + g.view(-1, 1, 1) * r2


@pytest.mark.parametrize("nf,h,w,throughput", [(64, 180, 320, True), (64, 180, 320, False), (64, 36, 70, False), (32, 36, 70, True), (64, 2, 2, False)])
def test_whole_rcab_fold_on_and_off_vs_float64(e64, e32, nf, h, w, throughput):
    """(c) one RCAB through engine.rcab with the fold on and off, each against a float64 torch RCAB within the per-kernel bound of 3e-5
    on inputs of magnitude ~1 (outputs up to 5.7).  Measured on MI355X, fold on / off: 64 channels 180x320 throughput flow (Winograd-y
    conv.2) 1.97e-6 / 1.91e-6, latency flow (direct) 1.51e-6 / 1.62e-6; 36x70 1.34e-6 / 1.46e-6; 32 channels 36x70 1.26e-6 / 1.29e-6;
    2x2 3.6e-7 / 3.9e-7.  (2 = the fold in the latency flow too: the default, 1, folds in the throughput flow only.)"""
    sd, eng = _which(nf, e64, e32)
    x = torch.randn(nf, h, w, generator=torch.Generator().manual_seed(17))
    xd = cl(x)
    ref = _rcab64(sd, x)
    lq = torch.empty(7, 3, h, w, device=DEV)
    eng.nb = 1
    eng._set_flow(lq, throughput)
    eng._select(lq.shape, (4, 4))
    errs = {}
    was = eng.rcab_fold
    try:
        for fold in (True, False):
            eng.rcab_fold = 2 if fold else 0          # (2: folded in the latency flow too)
            out = torch.full((h, w, nf), float("nan"), device=DEV)
            eng.rcab(PFX, eng.full(xd), eng.full(out), h, w, "t_rcab")
            torch.cuda.synchronize()
            errs[fold] = float((out.cpu().permute(2, 0, 1).double() - ref).abs().max())
    finally:
        eng.rcab_fold = was
        eng._set_flow(lq, False)
    print(f"nf {nf} {h}x{w} throughput={throughput}: RCAB max-abs vs float64, fold on {errs[True]:.3e}, off {errs[False]:.3e} (|ref| max {float(ref.abs().max()):.2f})")
    assert errs[True] <= 3e-5 and errs[False] <= 3e-5


def test_kernel_is_independent_of_the_clip_count(e64):
    """(d, kernel) clip 2 of a 4-clip launch == the same clip launched alone, bit for bit (gate, bias, image; both forms)."""
    sd, eng = e64
    nf, h, w = 64, 30, 50
    lib = eng.lib
    clips = [_r1_and_partials(eng, nf, h, w, seed=40 + i) for i in range(4)]
    r1 = torch.stack([c[1] for c in clips]).contiguous()
    part = torch.stack([c[2] for c in clips]).contiguous()
    ent = eng.rcab_w[PFX]
    for wy in (False, True):
        master = ent["master_wy"] if wy else ent["master"]
        n = master.numel() * 2

        def run(r1p, partp, nclip):
            img = torch.zeros(nclip, n, dtype=torch.int16, device=DEV)
            bias, gate = torch.zeros(nclip, nf, device=DEV), torch.zeros(nclip, nf, device=DEV)
            from savsr_amd import _lib
            _lib.check(lib.savsr_rcab_gate_weights_batch(partp.data_ptr(), eng.pool_rows(h, w), 1.0 / (h * w), r1p.data_ptr(), h, w, nf, ent["a"].data_ptr(),
                                                         ent["cz"].data_ptr(), ent["w2"].data_ptr(), ent["b2"].data_ptr(), nf, ent["cm"], master.data_ptr(),
                                                         ent["bias"].data_ptr(), int(wy), 0, img.data_ptr(), bias.data_ptr(), gate.data_ptr(), nclip,
                                                         part[0].numel() * 4, r1[0].numel() * 4, n * 2, nf * 4, nf * 4, None), "rcab_gate_weights")
            torch.cuda.synchronize()
            return img, bias, gate
        i4, b4, g4 = run(r1, part, 4)
        i1, b1, g1 = run(r1[2], part[2], 1)
        assert torch.equal(i4[2], i1[0]) and torch.equal(b4[2], b1[0]) and torch.equal(g4[2], g1[0])
        assert not torch.equal(g4[2], g4[1])


@pytest.mark.parametrize("h,w", [(24, 40), (80, 160)])
def test_clip_alone_and_in_a_group_on_either_stream(e64, h, w):
    """(d) a whole frame of the throughput flow: the same clip alone and as clip 2 of a 4-clip launch sequence, on the engine's stream and
    on a sibling engine's, bitwise equal (80x160: conv.2 of the RCABs takes the Winograd-y image, 24x40 the direct one)."""
    sd, eng = e64
    sc = (2.0, 2.0)
    lq = synth.synth_clip(7, 3, h, w, seed=21, batch=4).to(DEV).contiguous()
    H, W = 2 * h, 2 * w
    o4 = torch.empty(4, 3, H, W, device=DEV)
    eng.forward_one(lq, sc, o4, throughput=True)
    torch.cuda.synchronize()
    o1 = torch.empty(3, H, W, device=DEV)
    eng.forward_one(lq[2].contiguous(), sc, o1, throughput=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o4).all())
    assert torch.equal(o4[2], o1)
    sib = eng.clone_for_stream()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    o1s = torch.empty(3, H, W, device=DEV)
    with torch.cuda.stream(side):
        sib.forward_one(lq[2].contiguous(), sc, o1s, throughput=True)
    side.synchronize()
    assert torch.equal(o1s, o1)
    assert torch.equal(sib.rcab_scr["gate"], eng.rcab_scr["gate"])       # (the last RCAB's gate of that clip, on both streams)


def test_stale_lds_does_not_leak(e64):
    """(e) the kernel stages its reductions through LDS: with every CU's LDS full of NaN patterns beforehand (a Winograd conv launch over
    NaN inputs, the trick of test_satu_hr_lanes_beyond_the_image_do_not_leak) gate, bias and image stay finite and bit-identical to an
    undisturbed run -- every LDS float the kernel reads was written by it."""
    from savsr_amd import _lib as L
    sd, eng = e64
    xnan = torch.full((180, 320, 64), float("nan"), device=DEV)
    sink = [torch.empty(180, 320, 64, device=DEV) for _ in range(6)]
    key = "RG.0.residual_group.0.rcab.0"

    def poison_lds():
        eng.nb = 1
        algo = eng.conv_algo
        eng.conv_algo = L.CONV_DIRECT_THROUGHPUT
        try:
            eng.conv_launch([eng.conv_desc(key, [eng.full(xnan)], eng.full(o), 180, 320) for o in sink], "poison")      # 720 Winograd tiles: every CU
        finally:
            eng.conv_algo = algo
    scr = eng.rcab_scr
    for h, w in [(17, 33), (180, 320), (36, 70)]:
        r1, r1d, part = _r1_and_partials(eng, 64, h, w, seed=3)
        for wy in (False, True):
            res = []
            for poison in (False, True):
                for t in scr.values():
                    t.zero_()
                if poison:
                    poison_lds()
                _launch(eng, r1d, part, h, w, wy)
                res.append([scr[k].clone() for k in ("gate", "bias", "wimg")])
            assert all(bool(torch.isfinite(t).all()) for t in res[1][:2])
            n = (eng.rcab_w[PFX]["master_wy"] if wy else eng.rcab_w[PFX]["master"]).numel() * 2
            assert bool(torch.isfinite(res[1][2][:n].view(torch.bfloat16).float()).all())
            assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))
