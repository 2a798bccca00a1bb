"""The sequence path on the host: harness.window_indices against the REFERENCE's generate_frame_indices lists, the CPU oracle run per
window against the REFERENCE's outputs on short videos (tests/golden/video_outputs.npz, tools/gen_golden_video.py), the argument checks
of SAVSR.upscale_video / VideoUpscaler (all of them raise before the GPU is touched) and the CLI's argument parsing."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import savsr_oracle as O
from savsr_amd.harness import window_indices
from savsr_amd.utils import synth
from tests.video_cases import INDEX_MAX_N, INDEX_NUM_FRAMES, PADDINGS, VIDEO_CASES, VIDEO_SEED, WEIGHT_SEED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vgold():
    return np.load(os.path.join(ROOT, "tests", "golden", "video_outputs.npz"))


def _net(**cfg):
    from savsr_amd.archs.savsr_arch import SAVSR
    return SAVSR(**cfg).eval()


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("nf", INDEX_NUM_FRAMES)
def test_window_indices_equal_the_reference_lists(vgold, padding, nf):
    from savsr_amd.video import check_length
    valid = 0
    for n in range(1, INDEX_MAX_N + 1):
        ref = vgold[f"idx/{padding}/{nf}/{n}"]
        got = np.array([window_indices(i, n, nf, padding) for i in range(n)], dtype=np.int32)
        assert np.array_equal(got, ref), (padding, nf, n)
        inside = bool(ref.min() >= 0 and ref.max() < n)
        if inside:
            valid += 1
            check_length(n, nf, padding)
        else:                       # the refusal upscale_video / VideoUpscaler.finish give, in datasets.py's words
            with pytest.raises(ValueError, match=f"video has {n} frames: too few for a {nf}-frame '{padding}' window"):
                check_length(n, nf, padding)
    assert valid >= 3


@pytest.mark.parametrize("name,cfg,n,h,w,sc,padding", VIDEO_CASES)
def test_oracle_per_window_vs_reference_golden(vgold, name, cfg, n, h, w, sc, padding):
    net = _net(**cfg)
    sd = synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=WEIGHT_SEED)
    video = synth.synth_clip(n, cfg.get("num_in_ch", 3), h, w, seed=VIDEO_SEED)[0]
    gold = torch.from_numpy(vgold[f"{name}/sr"])
    nt = torch.get_num_threads()
    torch.set_num_threads(8)                     # (the goldens' thread count: the oracle's reductions follow it)
    try:
        with torch.no_grad():
            for i in range(n):
                win = window_indices(i, n, net.num_frame, padding)
                sr = O.forward(sd, video[win][None], sc, cfg=net.cfg)
                assert float((sr[0] - gold[i]).abs().max()) <= 1e-6, (name, i)
    finally:
        torch.set_num_threads(nt)


def _u8(n, h=8, w=10, c=3):
    return torch.zeros(n, h, w, c, dtype=torch.uint8)


@pytest.mark.parametrize("kwargs,frames,match", [
    (dict(padding="mirror"), _u8(9), "padding = 'mirror' is not a mode"),
    (dict(out="uint16"), _u8(9), "out = 'uint16'"),
    (dict(scale=(2, 3, 4)), _u8(9), "scale must be a number or an"),
    (dict(scale=-2), _u8(9), "scale must be positive"),
    (dict(), _u8(3), "video has 3 frames: too few for a 7-frame 'reflection' window"),
    (dict(padding="circle"), _u8(6), "video has 6 frames: too few for a 7-frame 'circle' window"),
    (dict(), _u8(9, c=1), "frames have 1 channels, the network takes num_in_ch = 3"),
    (dict(), torch.zeros(9, 3, 8, 10), "float frames must be on the GPU"),
    (dict(), torch.zeros(9, 8, 10, 3, dtype=torch.int32), "frames must be uint8 or float"),
    (dict(), torch.zeros(8, 10, 3, dtype=torch.uint8), "got 3 dimensions"),
    (dict(), _u8(9, h=1), "SAVSR needs h, w >= 2"),
])
def test_upscale_video_refuses_bad_arguments_without_a_gpu(kwargs, frames, match):
    net = _net()                                  # (on the host: a check that let anything through would fail on the GPU-only engine)
    with pytest.raises(ValueError, match=match):
        net.upscale_video(frames, **kwargs)


def test_upscale_video_refuses_a_network_in_training_mode_and_on_the_host():
    net = _net()
    net.train()
    with pytest.raises(RuntimeError, match="call .eval"):
        net.upscale_video(_u8(9))
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        _net().upscale_video(_u8(9))


def test_video_upscaler_refuses_bad_arguments_without_a_gpu():
    from savsr_amd import VideoUpscaler
    with pytest.raises(ValueError, match="padding = 'zero'"):
        VideoUpscaler(_net(), 4, "zero")
    with pytest.raises(ValueError, match="out = 'png'"):
        VideoUpscaler(_net(), 4, out="png")
    up = VideoUpscaler(_net(), (2, 3))
    assert up.scale == (2.0, 3.0)
    with pytest.raises(ValueError, match="frames have 2 channels"):
        up.push(_u8(2, c=2))
    with pytest.raises(ValueError, match="float frames must be on the GPU"):
        up.push(torch.zeros(2, 3, 8, 10))
    with pytest.raises(ValueError, match="the video has no frames"):
        up.finish()
    assert VideoUpscaler(_net(num_in_ch=1), 4).T == 7


@pytest.mark.parametrize("padding", PADDINGS)
def test_streaming_readiness_never_needs_a_frame_not_pushed_yet(padding):
    """A frame push() returns has the window upscale_video gives it for every length the video can still turn out to have; the frames the
    upscaler keeps cover every window it has not returned yet."""
    from savsr_amd.video import VideoUpscaler
    up = VideoUpscaler.__new__(VideoUpscaler)
    up.T, up.half, up.padding, up.done = 7, 3, padding, 0
    for seen in range(1, 30):
        up.seen = seen
        upto = up.done
        while upto < seen and up._ready(upto):
            upto += 1
        for i in range(up.done, upto):
            mine = window_indices(i, upto + up.half + 1, up.T, padding)
            for n in range(seen, seen + 10):
                if all(0 <= j < n for i2 in range(n) for j in window_indices(i2, n, up.T, padding)):
                    assert window_indices(i, n, up.T, padding) == mine
        up.done = upto
        lo = up._keep_from()
        assert seen - lo <= (up.T if "circle" in padding else up.T - 1)
        for i in range(up.done, seen):
            for n in range(seen, seen + 10):
                if all(0 <= j < n for i2 in range(n) for j in window_indices(i2, n, up.T, padding)):
                    assert min(window_indices(i, n, up.T, padding)) >= lo


def test_cli_arguments():
    from savsr_amd.upscale import parse_args
    a = parse_args(["-i", "in", "-o", "out", "--scale", "4", "--checkpoint", "x.pth"])
    assert a.scale == (4.0, 4.0) and a.padding == "reflection" and a.checkpoint == "x.pth" and a.opt is None
    a = parse_args(["-i", "in", "-o", "out", "--scale", "3.5", "2", "--padding", "circle", "--opt", "t.yml"])
    assert a.scale == (3.5, 2.0) and a.padding == "circle" and a.opt == "t.yml"
    for bad in (["-i", "in", "-o", "out", "--scale", "4"],                                             # no network
                ["-i", "in", "-o", "out", "--scale", "4", "--opt", "a", "--checkpoint", "b"],       # both
                ["-i", "in", "-o", "out", "--scale", "1", "2", "3", "--checkpoint", "b"],
                ["-i", "in", "-o", "out", "--scale", "4", "--padding", "zero", "--checkpoint", "b"],
                ["-o", "out", "--scale", "4", "--checkpoint", "b"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_cli_help_runs():
    r = subprocess.run([sys.executable, "-m", "savsr_amd.upscale", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--scale" in r.stdout and "--padding" in r.stdout and "--checkpoint" in r.stdout
