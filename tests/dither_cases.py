"""What tests/test_dither.py (CPU) and tests/test_gpu_dither.py share: the inputs and the shapes of the dither tests."""
import numpy as np

# i of the constant fields t = i + j / 256 (k = 1, 4, 16: the depths 8, 10, 12), and integer codes that must pass unchanged
CONSTANT_I = sorted({0, 1, 16, 128, 234, 254} | {235 * k - 1 for k in (1, 4, 16)} | {240 * k - 1 for k in (1, 4, 16)})
EXACT_CODES = (0, 16, 235, 255, 940, 3760, 4095)

# savsr_video_quantize_u8_d: (H, W, c, frames, bytes the output lies off its alignment)
U8_CASES = [
    (8, 6, 3, 2, 0),        # vector path (48 pixels) whose 16-pixel runs span three rows
    (32, 48, 2, 2, 0),      # vector path, more than one period both ways
    (17, 33, 3, 2, 0),      # scalar path, wraps in x and y
    (16, 16, 1, 2, 0),
    (1, 1, 3, 2, 0),
    (8, 6, 3, 2, 1),        # the scalar path forced by the output pointer
    (5, 40, 3, 2, 0),       # two frames: blockIdx.y (as every case)
]
# savsr_video_quantize_yuvs_d: tests/test_gpu_yuv_siting.py's shapes, (H, W, samples the frames lie off their alignment)
YUV_CASES = [(6, 16, 0), (36, 64, 0), (1, 4, 0), (2, 4, 0), (1, 1, 0), (2, 2, 0), (5, 3, 0), (7, 6, 0), (30, 35, 0), (6, 16, 1)]
LUMA_CASES = [(6, 16), (36, 64), (5, 3), (30, 35)]
DEPTHS = (8, 10, 12)


def colours(depth):
    return (0, 1, 2, 3) if depth == 8 else (0, 1)         # 10 and 12 bits: the limited-range ids


def sitings(chroma):
    return {"420": (None, "left", "topleft"), "422": (None, "left"), "444": (None,)}[chroma]


def float_in(n, c, H, W, seed=0):
    """[n, c, H, W] float32, random in -0.2 .. 1.2 with 3 % NaN and one inf (the inputs of tests/test_gpu_yuv_siting.py)."""
    rng = np.random.RandomState(H * 3 + W + 7 * c + seed)
    x = rng.uniform(-0.2, 1.2, size=(n, c, H, W)).astype(np.float32)
    x[rng.uniform(size=x.shape) < 0.03] = np.nan
    x[n - 1, c // 2, 0, 0] = np.nan
    x[0, c - 1, H - 1, W - 1] = np.inf
    return x


def ramp(h=32, w=512):
    """One frame whose three channels ramp from 100 / 255 to 102 / 255 along x: two codes over 512 pixels."""
    r = ((np.float32(100) + np.float32(2) * np.arange(w, dtype=np.float32) / np.float32(w)) / np.float32(255)).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(r, (1, 3, h, w)))


def block_means(a):
    """Means of the aligned 16 x 16 blocks of [..., H, W] (H, W multiples of 16), float64."""
    a = np.asarray(a, dtype=np.float64)
    H, W = a.shape[-2:]
    return a.reshape(a.shape[:-2] + (H // 16, 16, W // 16, 16)).mean(axis=(-3, -1))


def corners(h=16, w=32):
    """The eight corner colours of the RGB cube, one frame each, tiled h x w: [8, 3, h, w] float32."""
    c = np.array([[(i >> 2) & 1, (i >> 1) & 1, i & 1] for i in range(8)], np.float32)
    return np.ascontiguousarray(np.broadcast_to(c[:, :, None, None], (8, 3, h, w)))
