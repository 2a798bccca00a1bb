"""The temporal denoiser's specification (savsr_amd/denoise.py) on the CPU: the coverage condition of the shared generator
(tests/denoise_cases.py: every tap count and both stop reasons occur), the properties that follow from the rule, the comparisons at
exactly A / A + 1 and B / B + 1, the top of the range, videos shorter than the radius, a sample-by-sample restatement, the streaming
window's bound and any-chunking equality (the numpy model and prepass._LookAhead itself on host tensors), every refusal's wording, the
command line's parsing, the header / binding / library at ABI 50, and the sanitizer host check of the kernels' device functions."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import savsr_amd
from savsr_amd import _lib, yuv
from savsr_amd import denoise as dn
from savsr_amd.denoise import denoise_frames, denoise_matrix, stream_ranges
from tests.denoise_cases import COVER_SHAPE, DEPTHS, RADII, STRENGTH, TIGHT, cover_video, frames_for, lengths_for, walk_video

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------- coverage
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("r", RADII)
def test_the_generator_reaches_every_tap_count_and_both_stop_reasons(r, depth):
    """A condition, not a measurement: on the shared coverage video every k = 1 .. 2 r + 1 occurs, and both stop reasons for r >= 4.  At
    r <= 2 the B stop cannot fire with (4, 9) (two differences <= 4 sum to at most 8): r = 2 runs with (4, 5) as well; at r = 1 it cannot
    fire at all, since a <= b."""
    m = cover_video(r, depth)
    assert m.shape == (frames_for(r),) + COVER_SHAPE
    _, counts = denoise_matrix(m, r, *STRENGTH, depth, return_counts=True)
    assert counts["k"][0] == 0 and counts["k"].sum() == m.size
    assert all(counts["k"][k] > 0 for k in range(1, 2 * r + 2)), counts["k"]
    assert counts["stop_a"] > 0 and counts["stop_end"] > 0
    if r >= 4:
        assert counts["stop_b"] > 0
    else:
        assert counts["stop_b"] == 0
        _, tight = denoise_matrix(m, r, *TIGHT, depth, return_counts=True)
        assert (tight["stop_b"] > 0) == (r == 2)


def _naive(m, r, a, b, depth):
    """The rule, one sample at a time, in Python integers."""
    A, B, top = a << (depth - 8), b << (depth - 8), (1 << depth) - 1
    N, R, C = m.shape
    out = np.empty_like(m)
    for t in range(N):
        for y in range(R):
            for x in range(C):
                v = min(int(m[t, y, x]), top)
                total, k = v, 1
                for side in (-1, 1):
                    acc = 0
                    for d in range(1, r + 1):
                        u = t + side * d
                        if not 0 <= u < N:
                            break
                        tap = min(int(m[u, y, x]), top)
                        acc += abs(v - tap)
                        if abs(v - tap) > A or acc > B:
                            break
                        total, k = total + tap, k + 1
                out[t, y, x] = (total + (k >> 1)) // k
    return out


@pytest.mark.parametrize("depth", DEPTHS)
def test_the_vectorised_rule_is_the_rule_sample_by_sample(depth):
    for r, s in ((1, STRENGTH), (2, TIGHT), (4, STRENGTH), (4, (0, 0)), (16, (3, 200))):
        m = walk_video(np.random.default_rng(r + depth), min(frames_for(r), 14), 3, 20, depth)
        assert np.array_equal(denoise_matrix(m, r, *s, depth), _naive(m, r, *s, depth)), (r, s)


# ---------------------------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("depth", DEPTHS)
def test_properties_of_the_rule(depth):
    top = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    rng = np.random.default_rng(depth)
    static = np.repeat(rng.integers(0, top + 1, (1, 4, 9)), 7, 0).astype(dt)
    for r in RADII:
        assert np.array_equal(denoise_matrix(static, r, *STRENGTH, depth), static)          # a static sample, for every r
        m = cover_video(r, depth)
        A, B = STRENGTH[0] << (depth - 8), STRENGTH[1] << (depth - 8)
        out = denoise_matrix(m, r, *STRENGTH, depth)
        assert out.dtype == m.dtype and out.shape == m.shape
        assert np.abs(out.astype(np.int64) - m).max() <= min(A, B)                           # A and B bound how far a sample moves
        assert np.array_equal(denoise_matrix(m, r, 0, 0, depth), m)                          # (0, 0) averages exact repeats only
        loose = denoise_matrix(m, r, 255, 255, depth)
        assert np.abs(loose.astype(np.int64) - m).max() <= 255 << (depth - 8)
    # exact repeats of any length: runs of 1 .. 5 equal frames with far jumps between them
    runs = np.concatenate([np.full((n, 2, 3), v, dt) for n, v in ((1, 0), (3, top), (2, top // 2), (5, 7), (4, top - 9))])
    assert np.array_equal(denoise_matrix(runs, 4, *STRENGTH, depth), runs)
    # neighbours that all differ by more than A: unchanged, whatever B is
    A = 4 << (depth - 8)
    far = (np.arange(9).reshape(9, 1, 1) % 2 * (A + 1) + rng.integers(0, top - A, (1, 3, 5))).astype(dt)
    assert np.array_equal(denoise_matrix(far, 4, 4, 255, depth), far)
    # a jump: the first frame after it still averages forwards, the last one before it backwards
    jump = np.concatenate([np.full((4, 1, 1), 10, dt), np.array([100, 102, 101, 103], dt).reshape(4, 1, 1) << (depth - 8)])
    out, counts = denoise_matrix(jump, 4, *STRENGTH, depth, return_counts=True)
    assert int(out[4, 0, 0]) != int(jump[4, 0, 0]) and int(out[3, 0, 0]) == 10 and counts["k"][1] == 0


@pytest.mark.parametrize("depth", DEPTHS)
def test_comparisons_at_exactly_a_and_b(depth):
    sh = depth - 8
    a, b = 4, 9
    A, B = a << sh, b << sh
    x = 1000 >> (12 - depth)

    def first(samples, r=4):
        """Frame 0 of a one-sample video (its forward walk alone), and the last frame of the reversed one (the backward walk alone)."""
        m = np.array(samples).reshape(-1, 1, 1).astype(np.uint16 if sh else np.uint8)
        fwd = int(denoise_matrix(m, r, a, b, depth)[0, 0, 0])
        assert int(denoise_matrix(m[::-1], r, a, b, depth)[-1, 0, 0]) == fwd
        return fwd

    assert first([x, x + A]) == (2 * x + A + 1) // 2                  # diff == A: taken
    assert first([x, x + A + 1]) == x                                 # diff == A + 1: not
    assert first([x, x - A]) == (2 * x - A + 1) // 2 and first([x, x - A - 1]) == x
    # with (4, 9): two differences of A give acc = 8 u <= B; a third of u makes acc exactly B, of u + 1 (still <= A) B + 1
    u = 1 << sh
    assert B - 2 * A == u and u + 1 <= A
    assert first([x, x + A, x + A, x + u]) == (4 * x + 2 * A + u + 2) // 4          # acc == B: taken
    assert first([x, x + A, x + A, x + u + 1]) == (3 * x + 2 * A + 1) // 3         # acc == B + 1: the walk ends, the third tap is not taken
    assert first([x, x + A, x + A, x + u + 1, x]) == (3 * x + 2 * A + 1) // 3      # ... and a later exact repeat is not reached
    assert first([x, x + A, x - A, x + u]) == (4 * x + u + 2) // 4                  # acc sums absolute differences, whatever their signs


def test_the_top_of_the_range_and_every_divisor():
    """All samples 2^d - 1 at radius 16: n frames give k = n up to 17 and 17 .. 33 at n = 38, the sums are the largest the kernels see,
    and samples above the depth's range count as the largest one.  The kernels divide by a multiply with ceil(2^32 / k) and a shift: that
    arithmetic is exact for every sum they can see."""
    for depth in DEPTHS:
        top = (1 << depth) - 1
        seen = np.zeros(34, np.int64)
        for n in list(range(1, 18)) + [38]:
            m = np.full((n, 2, 3), top, np.uint8 if depth == 8 else np.uint16)
            out, counts = denoise_matrix(m, 16, 255, 255, depth, return_counts=True)
            assert np.array_equal(out, m)
            seen += counts["k"]
        assert all(seen[1:34] > 0)
    over = np.full((5, 1, 2), 0xFFFF, np.uint16)
    assert (denoise_matrix(over, 2, *STRENGTH, 10) == 1023).all() and (denoise_matrix(over, 2, *STRENGTH, 12) == 4095).all()
    n = np.arange(33 * 4095 + 17, dtype=np.uint64)
    for k in range(2, 34):
        assert np.array_equal((n * np.uint64(((1 << 32) + k - 1) // k)) >> np.uint64(32), n // np.uint64(k)), k


@pytest.mark.parametrize("n", [1, 2, 3])
def test_videos_shorter_than_the_radius(n):
    for depth in DEPTHS:
        m = walk_video(np.random.default_rng(n), n, 3, 17, depth)
        for r in (4, 16):
            out, counts = denoise_matrix(m, r, *STRENGTH, depth, return_counts=True)
            assert np.array_equal(out, _naive(m, r, *STRENGTH, depth))
            assert counts["k"][n + 1:].sum() == 0
    one = walk_video(np.random.default_rng(9), 1, 3, 17)
    assert np.array_equal(denoise_matrix(one, 4), one)


def test_denoise_frames_over_every_plane():
    rng = np.random.default_rng(5)
    rgb = walk_video(rng, 8, 6, 7 * 3).reshape(8, 6, 7, 3)
    assert np.array_equal(denoise_frames(rgb), denoise_matrix(rgb.reshape(8, 6, 21), 4, 4, 9).reshape(rgb.shape))
    h, w = 7, 9
    for fmt, layout, depth in (("i420", "420", 8), ("i422", "422", 10), ("i444", "444", 12), ("y400", "400", 8)):
        planes = [walk_video(rng, 8, *hw, depth) for hw in ([(h, w)] + ([] if layout == "400" else [yuv.chroma_hw(h, w, layout)] * 2))]
        frames = np.concatenate([(p.astype("<u2").view(np.uint8) if depth > 8 else p).reshape(8, -1) for p in planes], 1)
        assert frames.shape[1] == yuv.frame_bytes(h, w, depth, layout)
        got = denoise_frames(frames, fmt, (h, w), depth, 2, (4, 9), (2, 3))
        want = [denoise_matrix(p, 2, *((4, 9) if i == 0 else (2, 3)), depth) for i, p in enumerate(planes)]
        want = np.concatenate([(p.astype("<u2").view(np.uint8) if depth > 8 else p).reshape(8, -1) for p in want], 1)
        assert np.array_equal(got, want), fmt
        assert np.array_equal(denoise_frames(frames, fmt, (h, w), depth, 2, (4, 9)), denoise_frames(frames, fmt, (h, w), depth, 2, (4, 9), (4, 9)))
    assert np.array_equal(denoise_frames(torch.from_numpy(rgb)), denoise_frames(rgb))


# ---------------------------------------------------------------------------------------------------------------------- streaming
CHUNKINGS = ([1] * 20, [2] * 10, [5] * 4, [20], [3, 0, 1, 9, 0, 7], [19, 1], [1, 19])


@pytest.mark.parametrize("r", [1, 2, 4, 16])
def test_the_streaming_model_is_bounded_and_equals_the_whole_video(r):
    """The numpy model of TemporalDenoiser's indexing: the ranges tile the video, every range has r frames of context on either side
    wherever the video has them, at most 2 r frames stay between pushes, and the rule on each buffer gives the whole video's frames."""
    video = walk_video(np.random.default_rng(r), 20, 2, 9)
    whole = denoise_matrix(video, r, *STRENGTH)
    for chunks in CHUNKINGS:
        done, parts = 0, []
        steps = stream_ranges(chunks, r)
        for i, (first, count, lo, hi, held) in enumerate(steps):
            assert first + lo == done and held <= 2 * r
            if hi > lo:
                assert first + lo - r >= first or first == 0                                   # r frames behind, or the video's start
                assert i == len(steps) - 1 or first + hi + r <= first + count                  # r frames ahead, or the video's end
                parts.append(denoise_matrix(video[first:first + count], r, *STRENGTH)[lo:hi])
            done += hi - lo
        assert done == 20 and steps[-1][4] == 0
        assert np.array_equal(np.concatenate(parts), whole), chunks


@pytest.mark.parametrize("r", [1, 2, 4, 16])
def test_the_window_itself_follows_the_model(r):
    """prepass._LookAhead(r, r) on host tensors: the buffers, ranges and held counts of the model; (1, 1) is the window as it was."""
    from savsr_amd.prepass import _LookAhead
    video = torch.arange(20, dtype=torch.uint8).view(20, 1).repeat(1, 3)
    for chunks in CHUNKINGS:
        win, pushed = _LookAhead(r, r), 0
        steps = stream_ranges(chunks, r)
        for k, (first, count, lo, hi, held) in zip(chunks + [None], steps):
            buf, blo, bhi = win.take(None, True) if k is None else win.take(video[pushed:pushed + k])
            pushed += k or 0
            if buf is None:
                assert hi == lo
            else:
                assert (blo, bhi) == (lo, hi) and buf[:, 0].tolist() == list(range(first, first + count))
            assert win.held == held <= 2 * r
    assert (_LookAhead().ahead, _LookAhead().behind) == (1, 1)


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_are_worded():
    m = np.zeros((3, 2, 2), np.uint8)
    for r in (0, 17, -1, 2.0, True, None, "4"):
        with pytest.raises(ValueError, match=r"radius = .*: an int in 1 \.\. 16"):
            denoise_matrix(m, r)
    for s in ((5, 4), (-1, 3), (0, 256), (1, 2, 3), (1.0, 2), "4,9", None, (True, 2)):
        with pytest.raises(ValueError, match=r"strength = .*: \(a, b\) ints in 8-bit code units with 0 <= a <= b <= 255"):
            denoise_frames(np.zeros((3, 2, 2, 3), np.uint8), strength=s)
    with pytest.raises(ValueError, match=r"chroma_strength = \(9, 4\)"):
        denoise_frames(np.zeros((3, 6), np.uint8), "i420", (2, 2), chroma_strength=(9, 4))
    with pytest.raises(ValueError, match=r"\(a, b\) = \(5, 4\)"):
        denoise_matrix(m, 4, 5, 4)
    with pytest.raises(ValueError, match=r"matrices must be \[N, R, C\] integers"):
        denoise_matrix(np.zeros((3, 2, 2), np.float32))
    with pytest.raises(ValueError, match="the video has no frames"):
        denoise_matrix(np.zeros((0, 2, 2), np.uint8))
    with pytest.raises(ValueError, match="depth = 9: 8, 10 or 12"):
        denoise_matrix(m, depth=9)
    with pytest.raises(ValueError, match="float frames have no integer samples to denoise"):
        denoise_frames(np.zeros((3, 2, 2, 3), np.float32))
    with pytest.raises(ValueError, match=r"frames must be \[N, h, w, c\] uint8"):
        denoise_frames(np.zeros((3, 2, 2), np.uint8))
    with pytest.raises(ValueError, match=r"I420 frames of 2 x 2 are \[N, 6\] uint8"):
        denoise_frames(np.zeros((3, 7), np.uint8), "i420", (2, 2))
    with pytest.raises(ValueError, match="depth = 10 goes with pixel_format"):
        denoise_frames(np.zeros((3, 2, 2, 3), np.uint8), depth=10)
    with pytest.raises(ValueError, match=r"denoise = 'nlmeans': None or one of ata"):
        dn.check_denoiser("nlmeans")
    assert dn.check_denoise_options(None, 4, (4, 9), None) is None and dn.check_denoise_options(None, 4, [4, 9], None) is None
    assert dn.check_denoise_options("ata", 2, (1, 2), None) == (2, (1, 2), (1, 2))
    assert dn.check_denoise_options("ata", 2, (1, 2), (0, 0)) == (2, (1, 2), (0, 0))
    assert (dn.DEFAULT_RADIUS, dn.DEFAULT_STRENGTH, dn.MAX_RADIUS) == (4, (4, 9), 16)


def test_the_video_calls_refuse_before_the_gpu_is_touched():
    """upscale_video / VideoUpscaler on a network that is not on a GPU: every refusal below is raised on the host, before the call would
    have asked for the device (a good call ends at that question)."""
    from savsr_amd import VideoUpscaler
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR(num_feat=32).eval()
    v = torch.zeros(8, 12, 16, 3, dtype=torch.uint8)
    calls = (lambda **kw: net.upscale_video(v, scale=2, out="uint8", **kw), lambda **kw: VideoUpscaler(net, 2, out="uint8", **kw))
    for call in calls:
        with pytest.raises(ValueError, match=r"denoise = 'hqdn3d': None or one of ata"):
            call(denoise="hqdn3d")
        with pytest.raises(ValueError, match=r"denoise = True: None or one of ata"):
            call(denoise=True)
        with pytest.raises(ValueError, match=r"denoise_radius = 2 goes with denoise="):
            call(denoise_radius=2)
        with pytest.raises(ValueError, match=r"denoise_strength = \(2, 3\) goes with denoise="):
            call(denoise_strength=(2, 3))
        with pytest.raises(ValueError, match=r"denoise_chroma_strength = \(4, 9\) goes with denoise="):
            call(denoise_chroma_strength=(4, 9))
        with pytest.raises(ValueError, match=r"denoise_radius = 17: an int in 1 \.\. 16"):
            call(denoise="ata", denoise_radius=17)
        with pytest.raises(ValueError, match=r"denoise_radius = 0: an int in 1 \.\. 16"):
            call(denoise="ata", denoise_radius=0)
        with pytest.raises(ValueError, match=r"denoise_strength = \(9, 4\): \(a, b\) ints"):
            call(denoise="ata", denoise_strength=(9, 4))
        with pytest.raises(ValueError, match=r"denoise_chroma_strength = \(0, 256\): \(a, b\) ints"):
            call(denoise="ata", denoise_chroma_strength=(0, 256))
    with pytest.raises(TypeError):                                                   # keyword only
        net.upscale_video(v, 2, "reflection", "uint8", "rgb", None, None, 10.0, "bt601", None, 8, None, None, None, None, None, 24, "keep", None,
                          None, 5, "ata")
    f = torch.zeros(8, 3, 12, 16)
    with pytest.raises(ValueError, match="float frames"):                            # (host float frames are no frames of any call; float frames
        net.upscale_video(f, scale=2, denoise="ata")                                 # on the GPU are refused by the stage: tests/test_gpu_denoise.py)
    with pytest.raises(ValueError, match="float frames"):
        VideoUpscaler(net, 2, denoise="ata").push(f)
    with pytest.raises(RuntimeError, match="AMD GPU only"):                          # a good call gets as far as the device
        net.upscale_video(v, scale=2, out="uint8", denoise="ata", denoise_radius=16, denoise_strength=(0, 255))
    with pytest.raises(ValueError, match="float frames have no integer samples to denoise"):
        savsr_amd.denoise_video(f)
    with pytest.raises(ValueError, match=r"radius = 0"):
        savsr_amd.denoise_video(v, radius=0)
    with pytest.raises(ValueError, match=r"chroma_strength = \(3, 2\)"):
        savsr_amd.denoise_video(v, chroma_strength=(3, 2))


# ---------------------------------------------------------------------------------------------------------------------- the CLI
def test_cli_arguments(capsys):
    from savsr_amd.upscale import denoise_kwargs, parse_args
    base = ["-i", "in.y4m", "-o", "out.y4m", "--scale", "2", "--checkpoint", "x.pth"]
    a = parse_args(base)
    assert a.denoise is None and denoise_kwargs(a) == {}
    assert denoise_kwargs(parse_args(base + ["--denoise", "none"])) == {}
    a = parse_args(base + ["--denoise", "ata"])
    assert denoise_kwargs(a) == dict(denoise="ata", denoise_radius=4, denoise_strength=(4, 9), denoise_chroma_strength=None)
    a = parse_args(base + ["--denoise", "ata", "--denoise-radius", "16", "--denoise-strength", "2, 30", "--denoise-chroma-strength", "0,0"])
    assert denoise_kwargs(a) == dict(denoise="ata", denoise_radius=16, denoise_strength=(2, 30), denoise_chroma_strength=(0, 0))
    png = ["-i", "in", "-o", "out", "--scale", "2", "--checkpoint", "x.pth"]
    assert denoise_kwargs(parse_args(png + ["--denoise", "ata", "--denoise-radius", "1"]))["denoise_radius"] == 1
    for extra, words in ((["--denoise-radius", "2"], "go with --denoise ata"),
                         (["--denoise-strength", "1,2"], "go with --denoise ata"),
                         (["--denoise", "none", "--denoise-chroma-strength", "1,2"], "go with --denoise ata"),
                         (["--denoise", "ata", "--denoise-radius", "17"], "--denoise-radius = 17: an int in 1 .. 16"),
                         (["--denoise", "ata", "--denoise-strength", "9,4"], "--denoise-strength = (9, 4)"),
                         (["--denoise", "ata", "--denoise-strength", "4"], "--denoise-strength: A,B, got '4'"),
                         (["--denoise", "ata", "--denoise-strength", "a,b"], "A,B with integers"),
                         (["--denoise", "ata", "--denoise-chroma-strength", "1,300"], "--denoise-chroma-strength = (1, 300)"),
                         (["--denoise", "nlmeans"], "invalid choice")):
        with pytest.raises(SystemExit):
            parse_args(base + extra)
        assert words in capsys.readouterr().err, extra
    with pytest.raises(SystemExit):
        parse_args(png + ["--denoise", "ata", "--denoise-chroma-strength", "1,2"])
    assert "goes with a Y4M input" in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------------------------------- the ABI
def test_header_binding_and_library_agree_at_abi_50():
    hdr = open(os.path.join(ROOT, "include", "savsr_hip.h")).read()
    assert int(re.search(r"#define\s+SAVSR_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 50
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    assert lib.savsr_abi_version() == _lib.ABI_VERSION
    for name in ("savsr_video_denoise_u8", "savsr_video_denoise_u16"):
        decl = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, plain, flags=re.S)
        assert decl, name
        params = [p.strip() for p in decl.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert len(params) == len(args), (name, params)
        for p, t in zip(params, args):          # pointers travel as void pointers, int64_t as c_int64, int as c_int
            want = _lib.C.c_void_p if "*" in p else _lib.C.c_int64 if p.startswith("int64_t") else _lib.C.c_int
            assert t is want, (name, p)
        assert hasattr(lib, name)
    names = [p.split()[-1].lstrip("*") for p in re.search(r"savsr_video_denoise_u16\s*\((.*?)\);", plain, flags=re.S).group(1).split(",")]
    assert names == ["frames", "n_frames", "frame_bytes", "plane_offset", "rows", "cols", "depth", "radius", "thr_a", "thr_b", "from", "to", "out",
                     "out_frame_bytes", "out_plane_offset", "stream"]
    assert "denoise.hip" in open(os.path.join(ROOT, "savsr_amd", "csrc", "build.sh")).read()
    assert callable(savsr_amd.denoise_video) and savsr_amd.denoise is dn


# ---------------------------------------------------------------------------------------------------------------------- the host check
CXX = os.environ.get("CXX") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++"))


@pytest.mark.skipif(not CXX, reason="no clang++: the sanitizer build of the device functions needs one")
def test_the_device_functions_pass_the_sanitizer_host_check():
    """tools/check_denoise_host.py: csrc/denoise.hip's device functions as a stand-alone host program under ASan / UBSan, against the
    specification (both forms, misaligned bases, planes inside frames, sub-ranges)."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_denoise_host.py"), "--cxx", CXX], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "cases equal the specification, no sanitizer report" in res.stdout
