"""Host side of the folded RCAB (savsr_rcab_gate_weights_batch): the mean of a zero-padded 3x3 conv's output from
the border form of its input's tap sums, the SE gate's first layer composed with the conv, and the fp32 master images the kernel
scales by the gate.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from savsr_amd import packing as P

SHAPES = [(2, 2), (2, 7), (7, 2), (3, 3), (4, 6), (5, 8), (9, 5), (16, 32), (17, 33), (180, 320)]


def _case(c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    r1 = torch.relu(torch.randn(c, h, w, generator=g, dtype=torch.float64))        # conv.0 ends in a ReLU
    wt = torch.randn(c, c, 3, 3, generator=g, dtype=torch.float64) * 0.05
    b = torch.randn(c, generator=g, dtype=torch.float64) * 0.1
    return r1, wt, b


@pytest.mark.parametrize("h,w", SHAPES)
def test_border_form_mean_equals_the_mean_of_the_conv(h, w):
    """b + W S / n with S from the border form == mean over pixels of F.conv2d(r1, W, b, padding=1), in float64 to 1e-12 relative."""
    c = 64 if (h, w) == (180, 320) else 16
    r1, wt, b = _case(c, h, w, seed=h * 1000 + w)
    ref = F.conv2d(r1[None], wt, b, padding=1)[0].mean((1, 2))
    s = P.tap_sums_border(r1)                                                       # [c][3][3]
    got = b + (wt * s[None]).sum((1, 2, 3)) / (h * w)
    rel = float((got - ref).abs().max() / ref.abs().max())
    assert rel <= 1e-12, rel


@pytest.mark.parametrize("h,w", [(2, 2), (3, 5), (6, 4)])
def test_border_form_equals_the_sum_over_the_pixels_a_tap_sees(h, w):
    """S[ci][ky][kx] against its definition: r1 zero-padded by one, summed over the h x w window at offset (ky, kx)."""
    r1, _, _ = _case(8, h, w, seed=3)
    pad = F.pad(r1, (1, 1, 1, 1))
    s = P.tap_sums_border(r1)
    for ky in range(3):
        for kx in range(3):
            ref = pad[:, ky:ky + h, kx:kx + w].sum((1, 2))
            assert float((s[:, ky, kx] - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("c,cmid", [(64, 4), (32, 2)])
def test_precomposed_first_layer_reproduces_w1_mean(c, cmid):
    """A S / n + cz (rcab_fold_tables, fp32 tables of float64 products) == w1 mean(conv.2(r1)) + b1 to the tables' fp32 rounding."""
    h, w = 12, 20
    r1, wt, b = _case(c, h, w, seed=c)
    g = torch.Generator().manual_seed(7)
    w1 = torch.randn(cmid, c, 1, 1, generator=g, dtype=torch.float64) * 0.2
    b1 = torch.randn(cmid, generator=g, dtype=torch.float64) * 0.1
    a, cz = P.rcab_fold_tables(wt.float(), b.float(), w1.float(), b1.float())
    assert a.shape == (cmid, c * 9) and a.dtype == torch.float32 and cz.shape == (cmid,)
    mean = F.conv2d(r1[None], wt.float().double(), b.float().double(), padding=1)[0].mean((1, 2))
    ref = w1.float().double().reshape(cmid, c) @ mean + b1.float().double()
    got = a.double() @ P.tap_sums_border(r1).reshape(-1) / (h * w) + cz.double()
    # fp32 rounding of the c * 9 table entries (2^-24 relative each) against sums of magnitude |a| |S| / n
    bound = 2.0 ** -23 * float((a.double().abs() @ P.tap_sums_border(r1).reshape(-1).abs()) .max() / (h * w)) + 2.0 ** -23 * float(cz.abs().max())
    assert float((got - ref).abs().max()) <= bound


def _split_sum(img: torch.Tensor) -> torch.Tensor:
    """hi + lo of a split-bf16 image [n][2][512] -> fp32 [n * 512]."""
    v = img.view(torch.bfloat16).view(-1, 2, 512).to(torch.float32)
    return (v[:, 0] + v[:, 1]).reshape(-1)


@pytest.mark.parametrize("c", [64, 32])
def test_master_images_are_consistent_with_the_static_images(c):
    """The fp32 master parts the kernel scales are the values the static images split: hi + lo == master to the split's rounding
    (lo = bf16(v - hi): |v - hi - lo| <= 2^-9 |v - hi| <= 2^-17 |v|), in the same element order; unaddressed entries are zero."""
    g = torch.Generator().manual_seed(c)
    wt = torch.randn(c, c, 3, 3, generator=g) * 0.05
    forms = [(P.pack_conv_part(wt), P.pack_conv_weight(wt))]
    if c % 64 == 0:
        forms.append((P.pack_conv_part_wy(wt), P.pack_conv_weight_wy(wt)))
    for master, img in forms:
        assert master.dtype == torch.float32 and master.numel() * 2 == img.numel()
        d = (_split_sum(img) - master).abs()
        assert bool((d <= 2.0 ** -17 * master.abs()).all())
    # the direct master holds W at savsr_conv_pack_index, the Winograd-y master the float64 transform rounded once
    idx, total = P.conv_pack_index(c, c, 3)
    assert torch.equal(forms[0][0][torch.from_numpy(idx)], wt.reshape(-1))
    if c % 64 == 0:
        idx, total = P.conv_wy_pack_index(c, c)
        u = torch.from_numpy(P.wy_transform_f64(wt)).to(torch.float32)
        assert torch.equal(forms[1][0][torch.from_numpy(idx)], u.reshape(-1))


def test_gate_of_the_fold_equals_the_gate_of_the_conv_output_fp32():
    """The whole identity in fp32 at the headline shape: the gate from the border form against a float64 gate of the fp32 conv's mean, and
    conv_{g W}(r1) + g b + x against g conv_W(r1) + x (the issue's CPU check: ~6e-8 and ~6e-7 on outputs of magnitude 5)."""
    c, cmid, h, w = 64, 4, 180, 320
    g = torch.Generator().manual_seed(11)
    x = torch.randn(c, h, w, generator=g)
    r1 = torch.relu(torch.randn(c, h, w, generator=g))
    wt = torch.randn(c, c, 3, 3, generator=g) * 0.04
    b = torch.randn(c, generator=g) * 0.1
    w1, b1 = torch.randn(cmid, c, generator=g) * 0.3, torch.randn(cmid, generator=g) * 0.1
    w2, b2 = torch.randn(c, cmid, generator=g) * 0.3, torch.randn(c, generator=g) * 0.1
    r2_64 = F.conv2d(r1.double()[None], wt.double(), b.double(), padding=1)[0]
    gate64 = torch.sigmoid(w2.double() @ torch.relu(w1.double() @ r2_64.mean((1, 2)) + b1.double()) + b2.double())
    a, cz = P.rcab_fold_tables(wt, b, w1, b1)
    s = P.tap_sums_border(r1)                                                       # fp32 sums
    gate = torch.sigmoid(w2 @ torch.relu(a @ s.reshape(-1) / (h * w) + cz) + b2)
    assert float((gate.double() - gate64).abs().max()) <= 1e-6
    out = F.conv2d(r1[None], wt * gate.view(-1, 1, 1, 1), gate * b, padding=1)[0] + x
    ref = gate64.view(-1, 1, 1) * r2_64 + x.double()
    assert float((out.double() - ref).abs().max()) <= 3e-5
