"""CPU checks of the spatial denoiser: the rule of savsr_amd/nlmeans.py and what follows from it, the weight table and the C side's copy
of it, the coverage of the shared case generator, noise reduction on a synthetic picture, option checks and refusal messages, the
command line's parsing, the stage's place in VideoUpscaler (stateless: no look-ahead), the header / binding / library at ABI 51, and the
sanitizer host check of the kernels' device functions."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import savsr_amd
from savsr_amd import _lib
from savsr_amd import nlmeans as nl
from tests.nlmeans_cases import COVER_SHAPE, DEPTHS, as_bytes, case_frames, case_plane, synthetic_picture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _naive(m, depth, P, S, D):
    """The rule sample by sample, straight from the module's docstring."""
    R, C = m.shape
    v = np.minimum(m.astype(np.int64), (1 << depth) - 1)
    out = np.empty_like(m)
    cl = lambda y, x: v[min(max(y, 0), R - 1), min(max(x, 0), C - 1)]          # noqa: E731
    for y in range(R):
        for x in range(C):
            sw = sv = 0
            for dy in range(-S, S + 1):
                for dx in range(-S, S + 1):
                    if not (0 <= y + dy < R and 0 <= x + dx < C):
                        continue
                    ssd = sum((cl(y + i, x + j) - cl(y + dy + i, x + dx + j)) ** 2 for i in range(-P, P + 1) for j in range(-P, P + 1))
                    k = ((ssd >> (2 * (depth - 8))) * 64) // D
                    w = nl.WEIGHTS[k] if k < 577 else 0
                    sw += w
                    sv += w * v[y + dy, x + dx]
            out[y, x] = (sv + (sw >> 1)) // sw
    return out


# ---------------------------------------------------------------------------------------------------------------------- the table
def test_the_weight_table_and_the_c_sides_copy():
    W = nl.WEIGHTS
    assert len(W) == nl.N_WEIGHTS == 577 and W[0] == 4096 and W[576] == 1 and all(w > 0 for w in W)
    assert all(isinstance(w, int) for w in W) and list(W) == sorted(W, reverse=True)
    exact = 4096.0 * np.exp(-np.arange(578) / 64.0)
    assert np.rint(exact[577]) == 0                                   # entry 577 would round to 0
    frac = np.abs(exact[:577] - np.floor(exact[:577]) - 0.5)
    assert frac.argmin() == 22 and 1.0e-3 < frac.min() < 1.2e-3        # no entry is near enough to a half for a libm to flip it
    hdr = open(os.path.join(ROOT, "savsr_amd", "csrc", "nlmeans_weights.hpp")).read()
    body = re.search(r"NLM_WEIGHTS\[NLM_N_WEIGHTS \+ 1\] = \{(.*?)\};", hdr, flags=re.S).group(1)
    lits = [int(t) for t in body.replace("\n", " ").split(",")]
    assert len(lits) == 578 and lits[577] == 0
    for i, (a, b) in enumerate(zip(lits, W)):                         # entry by entry
        assert a == b, i
    assert int(re.search(r"NLM_N_WEIGHTS = (\d+);", hdr).group(1)) == 577
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_nlmeans_weights
        assert gen_nlmeans_weights.text() == hdr                      # the committed header is the generator's text
    finally:
        sys.path.pop(0)


# ---------------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("depth", DEPTHS)
def test_the_vectorised_rule_is_the_rule_sample_by_sample(depth):
    rng = np.random.default_rng(depth)
    for (r, c), P, S, D in (((6, 7), 1, 2, 9 * 9), ((5, 9), 3, 3, 441), ((1, 6), 2, 7, 100), ((7, 1), 3, 1, 1), ((1, 1), 3, 7, 441)):
        m = case_plane(rng, r, c, depth, above=True)
        assert np.array_equal(nl.nlm_matrix(m, depth, P, S, D), _naive(m, depth, P, S, D)), (r, c, P, S, D)


def test_the_generator_reaches_every_kind_of_bucket():
    """tests/nlmeans_cases.py `case_plane` on 24 x 40 at the defaults: candidates with k = 0 away from the centre, with a middle bucket
    (a weight strictly between 1 and 4096) and with k >= 577 (weight 0), at every depth."""
    for depth in DEPTHS:
        m = case_plane(np.random.default_rng(depth), *COVER_SHAPE, depth)
        _, counts = nl.nlm_matrix(m, depth, 3, 7, nl.divisor(3, 3.0), True)
        k = counts["k"]
        assert k.shape == (578,) and counts["k0_off_centre"] > 0 and k[0] == counts["k0_off_centre"] + m.size
        assert k[100:500].sum() > 0 and k[577] > 0 and k[1:577].sum() > 0, depth
        inside = sum(len(range(max(-7, -y), min(7, COVER_SHAPE[0] - 1 - y) + 1)) for y in range(COVER_SHAPE[0])) * \
            sum(len(range(max(-7, -x), min(7, COVER_SHAPE[1] - 1 - x) + 1)) for x in range(COVER_SHAPE[1]))
        assert k.sum() == inside                                      # every candidate inside the plane is counted once, zero weights included


@pytest.mark.parametrize("depth", DEPTHS)
def test_properties_of_the_rule(depth):
    rng = np.random.default_rng(10 + depth)
    top = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    for value in (0, 77, top):                                        # a constant plane comes back unchanged
        m = np.full((9, 11), value, dt)
        assert np.array_equal(nl.nlm_matrix(m, depth, 3, 7, 441), m)
    m = case_plane(rng, 20, 26, depth)
    P, S, D = 2, 3, nl.divisor(2, 4.0)
    out = nl.nlm_matrix(m, depth, P, S, D)
    assert out.dtype == m.dtype and not np.array_equal(out, m)
    # every output lies within the min / max of its candidates (the samples within S inside the plane)
    v = m.astype(np.int64)
    for y in range(20):
        for x in range(26):
            win = v[max(y - S, 0):y + S + 1, max(x - S, 0):x + S + 1]
            assert win.min() <= out[y, x] <= win.max(), (y, x)
    # exact equivariance under the flips and the transpose
    for f in (np.flipud, np.fliplr, np.transpose):
        assert np.array_equal(nl.nlm_matrix(np.ascontiguousarray(f(m)), depth, P, S, D), f(out)), f.__name__
    # translation invariance at distance >= S + P from the border: a window of the plane filtered alone agrees there
    sub = nl.nlm_matrix(m[3:, 4:], depth, P, S, D)
    e = S + P
    assert np.array_equal(sub[e:-e, e:-e], out[3 + e:-e, 4 + e:-e])
    # ... and not at the border: the rule does not commute with a crop
    assert not np.array_equal(sub, out[3:, 4:])
    # D = 1 on a plane without two equal patches is the identity: every other candidate has (SSD >> shift) * 64 >= 577 and weighs 0
    plane = ((rng.permutation(20 * 26).reshape(20, 26) % 200) << (depth - 8)).astype(dt)
    got, counts = nl.nlm_matrix(plane, depth, 1, 3, 1, True)
    assert counts["k"][:577].sum() == plane.size and counts["k"][0] == plane.size          # (only the centres weigh: the premise)
    assert np.array_equal(got, plane)


def test_noise_reduction_on_a_synthetic_picture():
    """48 x 64, clean 128 + 60 sin(x / 5) cos(y / 7) + 40 [x > 32] plus default_rng(0).normal(0, 2), rounded to uint8: at the defaults the
    MSE against the clean picture falls by a factor >= 1.5 (measured: 4.06 -> 2.16, 1.88); on a flat plane with sigma = 2 noise the
    variance falls at least 20-fold."""
    clean, noisy = synthetic_picture()
    out = nl.nlm_matrix(noisy, 8, nl.DEFAULT_PATCH, nl.DEFAULT_SEARCH, nl.divisor(nl.DEFAULT_PATCH, nl.DEFAULT_STRENGTH))
    before, after = float(((noisy - clean) ** 2).mean()), float(((out - clean) ** 2).mean())
    print(f"MSE {before:.3f} -> {after:.3f}: a factor {before / after:.3f}")
    assert before / after >= 1.5
    flat = np.clip(np.rint(128 + np.random.default_rng(0).normal(0, 2, (48, 64))), 0, 255).astype(np.uint8)
    res = nl.nlm_matrix(flat, 8, 3, 7, nl.divisor(3, 3.0))
    print(f"variance {flat.var():.4f} -> {res.var():.4f}")
    assert flat.var() >= 20 * res.var()
    assert nl.divisor(3, 3.0) == 441 and nl.divisor(1, 32) == 9216 and nl.divisor(3, 32) == 50176


def test_nlm_frames_over_every_plane_and_channel():
    rng = np.random.default_rng(3)
    v = case_frames(rng, 2, 6, 9, step=3)
    out = nl.nlm_frames(v, patch=1, search=2, strength=5)
    assert out.shape == v.shape and out.dtype == np.uint8
    for t in range(2):
        for ch in range(3):                                           # a channel only meets itself
            assert np.array_equal(out[t, :, :, ch], nl.nlm_matrix(v[t, :, :, ch], 8, 1, 2, nl.divisor(1, 5)))
    from savsr_amd import yuv
    for fmt, layout, depth, (h, w) in (("i420", "420", 8, (7, 9)), ("i422", "422", 10, (4, 6)), ("i444", "444", 12, (3, 5)), ("y400", "400", 8, (5, 4))):
        sizes = [(h, w)] + ([] if layout == "400" else [yuv.chroma_hw(h, w, layout)] * 2)
        planes = [case_frames(rng, 2, *hw, depth=depth)[..., 0] for hw in sizes]
        frames = np.concatenate([as_bytes(p) for p in planes], 1)
        out = nl.nlm_frames(frames, fmt, (h, w), depth, 2, 3, 4.0, 2.0)
        want = [np.stack([nl.nlm_matrix(p[t], depth, 2, 3, nl.divisor(2, 4.0 if i == 0 else 2.0)) for t in range(2)]) for i, p in enumerate(planes)]
        assert np.array_equal(out, np.concatenate([as_bytes(p) for p in want], 1)), fmt
        # stateless: every frame on its own, so any chunking of the video gives the same frames
        assert np.array_equal(np.concatenate([nl.nlm_frames(frames[t:t + 1], fmt, (h, w), depth, 2, 3, 4.0, 2.0) for t in range(2)]), out)
    with pytest.raises(ValueError, match="float frames have no integer samples to denoise"):
        nl.nlm_frames(np.zeros((1, 4, 4, 3), np.float32))
    with pytest.raises(ValueError, match=r"are \[N, 103\] uint8"):
        nl.nlm_frames(np.zeros((1, 90), np.uint8), "i420", (7, 9))


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_are_worded():
    for bad in (0, 4, True, 1.0, None):
        with pytest.raises(ValueError, match=r"patch = .*: an int in 1 \.\. 3"):
            nl.check_patch(bad)
    for bad in (0, 8, True, 2.0):
        with pytest.raises(ValueError, match=r"search = .*: an int in 1 \.\. 7"):
            nl.check_search(bad)
    for bad in (0, -1.0, 32.5, True, "3", None, float("nan"), (3, 4)):
        with pytest.raises(ValueError, match=r"strength = .*: a number with 0 < h <= 32"):
            nl.check_strength(bad)
    assert nl.check_strength(3) == 3.0 and nl.check_strength(np.float32(0.5)) == 0.5 and nl.check_strength(32) == 32.0
    with pytest.raises(ValueError, match=r"the divisor rint\(\(2 P \+ 1\)\^2 h\^2\) is 0, below 1"):
        nl.divisor(1, 0.2)
    with pytest.raises(ValueError, match="spatial_denoise = 'nlmeans': None or one of nlm"):
        nl.check_spatial_options("nlmeans", 3, 7, 3.0, None)
    with pytest.raises(ValueError, match="divisor = 0: an int >= 1"):
        nl.nlm_matrix(np.zeros((2, 2), np.uint8), 8, 3, 7, 0)
    with pytest.raises(ValueError, match="depth = 9"):
        nl.nlm_matrix(np.zeros((2, 2), np.uint8), 9)
    with pytest.raises(ValueError, match=r"must be \[R, C\] integers"):
        nl.nlm_matrix(np.zeros((2, 2), np.float32))
    assert nl.check_spatial_options(None, 3, 7, 3.0, None) is None and nl.check_spatial_options(None, 3, 7, 3, None) is None
    assert nl.check_spatial_options("nlm", 3, 7, 3.0, None) == (3, 7, 3.0, 3.0)
    assert nl.check_spatial_options("nlm", 1, 2, 4, 1.5) == (1, 2, 4.0, 1.5)
    assert (nl.DEFAULT_PATCH, nl.DEFAULT_SEARCH, nl.DEFAULT_STRENGTH, nl.MAX_SEARCH, nl.SPATIAL_DENOISERS) == (3, 7, 3.0, 7, ("nlm",))
    from savsr_amd import denoise as dn
    assert dn.DENOISERS == ("ata",)                                   # "nlmeans" stays an unknown denoise=
    with pytest.raises(ValueError, match="denoise = 'nlm': None or one of ata"):
        dn.check_denoise_options("nlm", 4, (4, 9), None)


def test_the_video_calls_refuse_before_the_gpu_is_touched():
    """upscale_video / VideoUpscaler on a network that is not on a GPU: every refusal below is raised on the host, before the call would
    have asked for the device (a good call ends at that question)."""
    from savsr_amd import VideoUpscaler
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR(num_feat=32).eval()
    v = torch.zeros(8, 12, 16, 3, dtype=torch.uint8)
    calls = (lambda **kw: net.upscale_video(v, scale=2, out="uint8", **kw), lambda **kw: VideoUpscaler(net, 2, out="uint8", **kw))
    for call in calls:
        with pytest.raises(ValueError, match=r"spatial_denoise = 'hqdn3d': None or one of nlm"):
            call(spatial_denoise="hqdn3d")
        with pytest.raises(ValueError, match=r"spatial_denoise = True: None or one of nlm"):
            call(spatial_denoise=True)
        with pytest.raises(ValueError, match=r"spatial_patch = 2 goes with spatial_denoise="):
            call(spatial_patch=2)
        with pytest.raises(ValueError, match=r"spatial_search = 5 goes with spatial_denoise="):
            call(spatial_search=5)
        with pytest.raises(ValueError, match=r"spatial_strength = 2\.0 goes with spatial_denoise="):
            call(spatial_strength=2.0)
        with pytest.raises(ValueError, match=r"spatial_chroma_strength = 3\.0 goes with spatial_denoise="):
            call(spatial_chroma_strength=3.0)
        with pytest.raises(ValueError, match=r"spatial_patch = 4: an int in 1 \.\. 3"):
            call(spatial_denoise="nlm", spatial_patch=4)
        with pytest.raises(ValueError, match=r"spatial_search = 8: an int in 1 \.\. 7"):
            call(spatial_denoise="nlm", spatial_search=8)
        with pytest.raises(ValueError, match=r"spatial_strength = 33: a number with 0 < h <= 32"):
            call(spatial_denoise="nlm", spatial_strength=33)
        with pytest.raises(ValueError, match=r"spatial_strength = 0\.1 with patch = 1: the divisor"):
            call(spatial_denoise="nlm", spatial_patch=1, spatial_strength=0.1)
        with pytest.raises(ValueError, match=r"spatial_chroma_strength = True: a number"):
            call(spatial_denoise="nlm", spatial_chroma_strength=True)
    with pytest.raises(TypeError):                                                   # keyword only
        VideoUpscaler(net, 2, "reflection", "uint8", "rgb", None, None, 10.0, "bt601", None, 8, None, None, None, None, None, "keep", None, None, 5,
                      "nlm")
    f = torch.zeros(8, 3, 12, 16)
    with pytest.raises(ValueError, match="float frames"):
        net.upscale_video(f, scale=2, spatial_denoise="nlm")
    with pytest.raises(ValueError, match="float frames"):
        VideoUpscaler(net, 2, spatial_denoise="nlm").push(f)
    with pytest.raises(RuntimeError, match="AMD GPU only"):                          # a good call gets as far as the device
        net.upscale_video(v, scale=2, out="uint8", spatial_denoise="nlm", spatial_patch=1, spatial_search=1, spatial_strength=32)
    with pytest.raises(ValueError, match="float frames have no integer samples to denoise"):
        savsr_amd.denoise_spatial(f)
    with pytest.raises(ValueError, match=r"patch = 0"):
        savsr_amd.denoise_spatial(v, patch=0)
    with pytest.raises(ValueError, match=r"chroma_strength = 40"):
        savsr_amd.denoise_spatial(v, chroma_strength=40)


def test_the_stage_in_video_upscaler_is_stateless():
    """The wiring needs no look-ahead: spatial_denoise= builds no streaming stage (nothing that holds frames back), only the checked
    options that `_take` applies to the frames it has cropped; the temporal denoiser, which does hold frames, is untouched by it."""
    from savsr_amd import VideoUpscaler
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR(num_feat=32).eval()
    up = VideoUpscaler(net, 2, out="uint8", spatial_denoise="nlm", spatial_patch=2, spatial_chroma_strength=1.0)
    assert up._grain == (2, 7, 3.0, 1.0) and up._noise is None and up._split is None and up._buf is None
    plain = VideoUpscaler(net, 2, out="uint8")
    assert plain._grain is None
    both = VideoUpscaler(net, 2, out="uint8", denoise="ata", denoise_radius=2, spatial_denoise="nlm")
    assert both._noise is not None and both._noise.radius == 2 and both._grain == (3, 7, 3.0, 3.0)


# ---------------------------------------------------------------------------------------------------------------------- the CLI
def test_cli_arguments(capsys):
    from savsr_amd.upscale import parse_args, spatial_kwargs
    base = ["-i", "in.y4m", "-o", "out.y4m", "--scale", "2", "--checkpoint", "x.pth"]
    a = parse_args(base)
    assert a.spatial_denoise is None and spatial_kwargs(a) == {}
    assert spatial_kwargs(parse_args(base + ["--spatial-denoise", "none"])) == {}
    a = parse_args(base + ["--spatial-denoise", "nlm"])
    assert spatial_kwargs(a) == dict(spatial_denoise="nlm", spatial_patch=3, spatial_search=7, spatial_strength=3.0, spatial_chroma_strength=None)
    a = parse_args(base + ["--spatial-denoise", "nlm", "--spatial-patch", "1", "--spatial-search", "2", "--spatial-strength", "4.5",
                           "--spatial-chroma-strength", "2"])
    assert spatial_kwargs(a) == dict(spatial_denoise="nlm", spatial_patch=1, spatial_search=2, spatial_strength=4.5, spatial_chroma_strength=2.0)
    png = ["-i", "in", "-o", "out", "--scale", "2", "--checkpoint", "x.pth"]
    assert spatial_kwargs(parse_args(png + ["--spatial-denoise", "nlm", "--spatial-search", "5"]))["spatial_search"] == 5
    a = parse_args(base + ["--denoise", "ata", "--spatial-denoise", "nlm"])          # the two stages go together
    assert a.denoise == "ata" and a.spatial_denoise == "nlm"
    for extra, words in ((["--spatial-patch", "2"], "go with --spatial-denoise nlm"),
                         (["--spatial-strength", "2"], "go with --spatial-denoise nlm"),
                         (["--spatial-denoise", "none", "--spatial-chroma-strength", "1"], "go with --spatial-denoise nlm"),
                         (["--spatial-denoise", "nlm", "--spatial-patch", "4"], "--spatial-patch = 4: an int in 1 .. 3"),
                         (["--spatial-denoise", "nlm", "--spatial-search", "0"], "--spatial-search = 0: an int in 1 .. 7"),
                         (["--spatial-denoise", "nlm", "--spatial-strength", "0"], "--spatial-strength = 0.0: a number with 0 < h <= 32"),
                         (["--spatial-denoise", "nlm", "--spatial-strength", "x"], "invalid float value"),
                         (["--spatial-denoise", "nlm", "--spatial-chroma-strength", "33"], "--spatial-chroma-strength = 33.0"),
                         (["--spatial-denoise", "nlm", "--spatial-patch", "1", "--spatial-strength", "0.1"], "the divisor"),
                         (["--spatial-denoise", "nlmeans"], "invalid choice")):
        with pytest.raises(SystemExit):
            parse_args(base + extra)
        assert words in capsys.readouterr().err, extra
    with pytest.raises(SystemExit):
        parse_args(png + ["--spatial-denoise", "nlm", "--spatial-chroma-strength", "2"])
    assert "goes with a Y4M input" in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------------------------------- the ABI
def test_header_binding_and_library_agree_at_abi_51():
    hdr = open(os.path.join(ROOT, "include", "savsr_hip.h")).read()
    assert int(re.search(r"#define\s+SAVSR_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 51
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    assert lib.savsr_abi_version() == _lib.ABI_VERSION
    for name in ("savsr_video_nlmeans_u8", "savsr_video_nlmeans_u16"):
        decl = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, plain, flags=re.S)
        assert decl, name
        params = [p.strip() for p in decl.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert len(params) == len(args), (name, params)
        for p, t in zip(params, args):          # pointers travel as void pointers, int64_t as c_int64, int as c_int
            want = _lib.C.c_void_p if "*" in p else _lib.C.c_int64 if p.startswith("int64_t") else _lib.C.c_int
            assert t is want, (name, p)
        assert hasattr(lib, name)
    names = [p.split()[-1].lstrip("*") for p in re.search(r"savsr_video_nlmeans_u16\s*\((.*?)\);", plain, flags=re.S).group(1).split(",")]
    assert names == ["frames", "n_frames", "frame_bytes", "plane_offset", "rows", "cols", "step", "depth", "patch", "search", "divisor", "out",
                     "out_frame_bytes", "out_plane_offset", "stream"]
    build = open(os.path.join(ROOT, "savsr_amd", "csrc", "build.sh")).read()
    assert build.count("nlmeans.hip") == 2 and "nlmeans_weights.hpp" in build
    assert callable(savsr_amd.denoise_spatial) and savsr_amd.nlmeans is nl
    # the entries refuse on the host, by name, before the device is touched
    assert lib.savsr_video_nlmeans_u8(0, 1, 1, 0, 1, 1, 1, 3, 7, 441, 0, 1, 0, None) == -1
    assert b"video_nlmeans_u8: null pointer" in lib.savsr_last_error()


# ---------------------------------------------------------------------------------------------------------------------- the host check
CXX = os.environ.get("CXX") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++"))


@pytest.mark.skipif(not CXX, reason="no clang++: the sanitizer build of the device functions needs one")
def test_the_device_functions_pass_the_sanitizer_host_check():
    """tools/check_nlmeans_host.py: csrc/nlmeans.hip's entries and shared device functions as a stand-alone host program under ASan /
    UBSan, against the specification (the tool's docstring says what the host form covers and what only the GPU tests do)."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_nlmeans_host.py"), "--cxx", CXX], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "cases equal the specification, no sanitizer report" in res.stdout
