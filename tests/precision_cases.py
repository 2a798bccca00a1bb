"""Case table of the precision-mode goldens, shared by tools/gen_golden_precision.py and tests/test_precision.py /
test_gpu_precision.py."""
from tests.golden_cases import NET_CASES

# (name, ctor kwargs, h, w, scale): the five NET_CASES on the shipped constructor, one num_feat = 32 and one num_in_ch = 1 case
PRECISION_CASES = [(name, {}, h, w, sc) for name, h, w, sc in NET_CASES] + [
    ("nf32_13x15_x3", dict(num_feat=32), 13, 15, (3, 3)),
    ("c1_12x14_x2p5", dict(num_in_ch=1), 12, 14, (2.5, 2.5)),
]
WEIGHT_SEED, CLIP_SEED = 0, 0
GT_CASE, GT_SEED = "cfg1_64x64_x2", 7          # the case whose dPSNR-Y is measured against a fixed synthetic GT


def psnr_y(sr, gt) -> float:
    """PSNR of the BT.601 luma (calculate_psnr(test_y_channel=True)'s Y, without the uint8 quantisation) of [3, H, W] RGB arrays in [0, 1]."""
    import numpy as np
    w = np.array([65.481, 128.553, 24.966]).reshape(3, 1, 1)
    ys = (np.asarray(sr, np.float64).clip(0, 1) * w).sum(0) + 16.0
    yg = (np.asarray(gt, np.float64).clip(0, 1) * w).sum(0) + 16.0
    return float(10.0 * np.log10(255.0 ** 2 / np.mean((ys - yg) ** 2)))


def synth_gt(fp32_out):
    """The fixed synthetic ground truth of GT_CASE: its fp32 output plus N(0, 0.02) noise (GT_SEED), clipped to [0, 1]."""
    import numpy as np
    n = np.random.RandomState(GT_SEED).standard_normal(np.shape(fp32_out))
    return np.clip(np.asarray(fp32_out, np.float64) + 0.02 * n, 0.0, 1.0).astype(np.float32)
