"""The precision mode "fp16" on the host (SAVSR.set_precision): the fp16 weight images, the mode's validation and persistence, the
refusal of weights outside the fp16 range, the CLI flags and the golden file's manifest."""
import os

import numpy as np
import pytest
import torch

from savsr_amd.utils import synth
from tests.golden_cases import manifest_hash
from tests.precision_cases import PRECISION_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _w(cout, cin, ks, seed, scale=1.0):
    return torch.from_numpy((scale * np.random.RandomState(seed).standard_normal((cout, cin, ks, ks))).astype(np.float32))


@pytest.mark.parametrize("cout,cin,ks", [(64, 64, 3), (128, 192, 3), (16, 16, 3), (1, 16, 3), (64, 64, 1), (32, 64, 3)])
def test_f16_direct_image(cout, cin, ks):
    from savsr_amd.packing import conv_pack_index, pack_conv_weight_f16
    w = _w(cout, cin, ks, cout + cin + ks)
    img = pack_conv_weight_f16(w).numpy().view(np.float16)
    idx, total = conv_pack_index(cout, cin, ks)
    assert img.shape == (total,)
    want = w.double().numpy().reshape(-1).astype(np.float16)
    assert np.array_equal(img[idx].view(np.int16), want.view(np.int16))
    rest = np.ones(total, bool)
    rest[idx] = False
    assert not img[rest].any()


@pytest.mark.parametrize("cout,cin", [(64, 64), (128, 320), (64, 16)])
def test_f16_winograd_image(cout, cin):
    from savsr_amd.packing import conv_wy_pack_index, pack_conv_weight_wy_f16
    w = _w(cout, cin, 3, 3 * cout + cin)
    img = pack_conv_weight_wy_f16(w).numpy().view(np.float16)
    idx, total = conv_wy_pack_index(cout, cin)
    g = w.double().numpy()
    g0, g1, g2 = g[:, :, 0], g[:, :, 1], g[:, :, 2]
    u = np.stack([g0, 0.5 * (g0 + g1 + g2), 0.5 * (g0 - g1 + g2), g2], 0)        # float64, rounded once
    assert np.array_equal(img[idx].view(np.int16), u.reshape(-1).astype(np.float16).view(np.int16))
    rest = np.ones(total, bool)
    rest[idx] = False
    assert not img[rest].any()


def test_set_precision_validation_and_state():
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR()
    assert net.precision == "fp32"
    keys = list(net.state_dict().keys())
    for bad in ("bf16", "FP16", "fp64", None, 16):
        with pytest.raises(ValueError):
            net.set_precision(bad)
    net.set_precision("fp16")
    assert net.precision == "fp16"
    assert list(net.state_dict().keys()) == keys and len(keys) == 791
    net.load_state_dict(synth.synth_state_dict(seed=1), strict=True)
    assert net.precision == "fp16"
    net = net.to(torch.float32).to("cpu")
    assert net.precision == "fp16"
    net.set_precision("fp32")
    assert net.precision == "fp32"


def test_f16_refuses_out_of_range_weights():
    from savsr_amd.packing import FP16_MAX, check_f16_range
    check_f16_range("ok", np.array([FP16_MAX, -FP16_MAX]))
    with pytest.raises(ValueError, match="conv 'RG.0.conv'"):
        check_f16_range("conv 'RG.0.conv'", np.array([1.0, -70000.0]))
    with pytest.raises(ValueError, match="fp16 range"):
        check_f16_range("x", np.array([np.inf]))


def test_engine_build_f16_names_the_conv():
    """_build_f16 on a packed engine's host-side state: the first static conv beyond +-65504 is named."""
    from savsr_amd.packing import WeightPacking
    sd = synth.synth_state_dict(seed=0)
    sd["h_win_conv_h.weight"] = sd["h_win_conv_h.weight"].clone()
    sd["h_win_conv_h.weight"][0, 0, 1, 1] = 1e5
    wp = WeightPacking.__new__(WeightPacking)
    wp._sd_ref, wp.pw16, wp.pw16_wy, wp.pw_wy, wp.osc, wp.cfg = sd, {}, {}, {}, {}, {"num_in_ch": 3, "slid_win": 3}
    wp._conv_src = {"conv_last": ("conv", "conv_last", None), "h_win_conv_h": ("conv", "h_win_conv_h", None)}
    with pytest.raises(ValueError, match="h_win_conv_h"):
        wp._build_f16()
    assert not wp.pw16                                     # nothing half-built


def test_cli_precision_flags():
    from savsr_amd.test import build_parser as test_parser
    from savsr_amd.upscale import build_parser as up_parser
    base = ["-i", "a", "-o", "b", "--scale", "4", "--checkpoint", "c.pth"]
    assert up_parser().parse_args(base).precision == "fp32"
    assert up_parser().parse_args(base + ["--precision", "fp16"]).precision == "fp16"
    with pytest.raises(SystemExit):
        up_parser().parse_args(base + ["--precision", "bf16"])
    assert test_parser().parse_args(["-opt", "x.yml"]).precision == "fp32"
    assert test_parser().parse_args(["-opt", "x.yml", "--precision", "fp16"]).precision == "fp16"
    with pytest.raises(SystemExit):
        test_parser().parse_args(["-opt", "x.yml", "--precision", "half"])


def test_run_test_rejects_bad_precision():
    from savsr_amd.test import run_test
    with pytest.raises(ValueError):
        run_test({}, precision="bf16")


def test_golden_manifest_and_drift():
    """The goldens were made on the manifests of the constructors they name; the emulated drift is small and non-zero."""
    from savsr_amd.archs.savsr_arch import SAVSR
    g = np.load(os.path.join(ROOT, "tests", "golden", "precision_outputs.npz"))
    assert manifest_hash(synth.manifest_of(SAVSR().state_dict())) == manifest_hash(synth.load_manifest())
    for name, kw, h, w, sc in PRECISION_CASES:
        assert str(g[f"{name}/manifest"]) == manifest_hash(synth.manifest_of(SAVSR(**kw).state_dict())), name
        c = SAVSR(**kw).cfg["num_in_ch"]
        assert g[f"{name}/fp32"].shape == (c, round(h * sc[0]), round(w * sc[1]))
        mx, mean = g[f"{name}/drift"]
        assert 0 < mean < mx < 2e-3
    assert abs(float(g["gt/psnr_fp16emu"]) - float(g["gt/psnr_fp32"])) < 0.01


def test_golden_clips_manifest_and_drift():
    """precision_clips.npz (tools/gen_golden_precision.py --clips): made on the shipped constructor's manifest; one fp32 output and one
    non-negative (max-abs, mean-abs) drift per clip that is not noise."""
    from savsr_amd.archs.savsr_arch import SAVSR
    g = np.load(os.path.join(ROOT, "tests", "golden", "precision_clips.npz"))
    assert str(g["manifest"]) == manifest_hash(synth.manifest_of(SAVSR().state_dict()))
    for clip in ("lowpass", "const", "zero"):
        assert g[f"{clip}/fp32"].shape == (3, round(13 * 2.5), round(18 * 3.5)) and g[f"{clip}/fp32"].dtype == np.float32
        assert bool(np.isfinite(g[f"{clip}/fp32"]).all())
        mx, mean = g[f"{clip}/drift"]
        assert 0 <= mean <= mx < 2e-3
    assert sorted(g.files) == sorted(["manifest"] + [f"{c}/{k}" for c in ("lowpass", "const", "zero") for k in ("fp32", "drift")])
