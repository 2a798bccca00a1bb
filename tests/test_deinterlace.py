"""The deinterlacer's specification (savsr_amd/deinterlace.py; no GPU): the vectorised rule against a scalar loop written from the rule's
text, its fixed points and symmetries, the branch-count guard of the shared inputs, the refusals and the CLI's header decision."""
import numpy as np
import pytest
import torch

from savsr_amd import yuv
from savsr_amd.deinterlace import (BRANCHES, FIELD_ORDERS, check_order, deinterlace_frames, deinterlace_frames_counted, deinterlace_matrix,
                                   resolve_fields)
from tests.deinterlace_cases import N_FRAMES, STEPS, input_set, shapes_for


# ---------------------------------------------------------------------------------------------------------------------- the scalar loop
def scalar_deinterlace(mats, order, step=1, depth=8):
    """The rule, one sample at a time, in Python integers; kept rows copied."""
    m = np.asarray(mats)
    N, R, C = m.shape
    top = (1 << depth) - 1
    v = [[[min(int(s), top) for s in row] for row in fr] for fr in m]
    out = np.repeat(m, 2, axis=0)
    s = step
    for n in range(N):
        cur, prev, nxt = v[n], v[max(n - 1, 0)], v[min(n + 1, N - 1)]
        for f in (0, 1):
            p = f if order == "tff" else 1 - f
            p2, n2 = (prev, cur) if f == 0 else (cur, nxt)
            for y in range(R):
                if y % 2 == p:
                    continue
                up = y - 1 if y > 0 else y + 1
                dn = y + 1 if y < R - 1 else y - 1
                for x in range(C):
                    c, e = cur[up][x], cur[dn][x]
                    d = (p2[y][x] + n2[y][x]) >> 1
                    t0 = abs(p2[y][x] - n2[y][x])
                    t1 = (abs(prev[up][x] - c) + abs(prev[dn][x] - e)) >> 1
                    t2 = (abs(nxt[up][x] - c) + abs(nxt[dn][x] - e)) >> 1
                    diff = max(t0 >> 1, t1, t2)
                    pred = (c + e) >> 1
                    if x - 3 * s >= 0 and x + 3 * s <= C - 1:
                        score = abs(cur[up][x - s] - cur[dn][x - s]) + abs(c - e) + abs(cur[up][x + s] - cur[dn][x + s]) - 1
                        for first in (-1, 1):
                            for j in (first, 2 * first):
                                sc = (abs(cur[up][x + (j - 1) * s] - cur[dn][x - (j + 1) * s]) + abs(cur[up][x + j * s] - cur[dn][x - j * s])
                                      + abs(cur[up][x + (j + 1) * s] - cur[dn][x - (j - 1) * s]))
                                if not sc < score:
                                    break
                                score, pred = sc, (cur[up][x + j * s] + cur[dn][x - j * s]) >> 1
                    if y - 2 >= 0 and y + 2 <= R - 1:
                        b = (p2[y - 2][x] + n2[y - 2][x]) >> 1
                        g = (p2[y + 2][x] + n2[y + 2][x]) >> 1
                        mx = max(d - e, d - c, min(b - c, g - e))
                        mn = min(d - e, d - c, max(b - c, g - e))
                        diff = max(diff, mn, -mx)
                    out[2 * n + f, y, x] = min(max(pred, d - diff), d + diff)
    return out


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_the_spec_equals_the_scalar_loop(order, step):
    for r, c in shapes_for(step):
        for name, v in input_set(r, c, step):
            got, _ = deinterlace_matrix(v, order, step)
            assert got.shape == (2 * N_FRAMES, r, c) and got.dtype == v.dtype
            assert np.array_equal(got, scalar_deinterlace(v, order, step)), (name, r, c, step, order)


@pytest.mark.parametrize("depth", [10, 12])
def test_the_spec_equals_the_scalar_loop_at_high_depth(depth):
    top = (1 << depth) - 1
    for name, v in input_set(9, 33, 1, top):
        v = v.astype(np.uint16)
        v[:, ::2, ::5] = 60000                                                       # above 2^d - 1, in rows of both parities
        v[:, 1::2, 3::7] = top + 1
        assert np.array_equal(deinterlace_matrix(v, "tff", 1, depth)[0], scalar_deinterlace(v, "tff", 1, depth)), (name, depth)


# ---------------------------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_kept_rows_are_copied(order):
    v = np.random.RandomState(3).randint(0, 256, size=(3, 9, 33)).astype(np.uint8)
    out, _ = deinterlace_matrix(v, order)
    for n in range(3):
        for f in (0, 1):
            p = f if order == "tff" else 1 - f
            assert np.array_equal(out[2 * n + f, p::2], v[n, p::2]), (order, n, f)
            assert not np.array_equal(out[2 * n + f, 1 - p::2], v[n, 1 - p::2])      # (noise: the other rows are not the woven ones)


def test_one_frame_is_its_own_prev_and_next():
    v = np.random.RandomState(4).randint(0, 256, size=(1, 9, 33)).astype(np.uint8)
    out, _ = deinterlace_matrix(v, "tff")
    assert out.shape == (2, 9, 33) and np.array_equal(out, scalar_deinterlace(v, "tff"))
    # prev = next = cur is what a static video of three frames gives its middle frame
    assert np.array_equal(out, deinterlace_matrix(np.repeat(v, 3, 0), "tff")[0][2:4])


@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_a_static_video_of_vertical_ramps_comes_back_as_itself(order):
    """Columns that are linear in y with slope m: d is the woven sample itself and every temporal difference is 0.  In the interior
    rows d - c = m = -(d - e) and b - c = -m = -(f - e), so mn <= 0 <= mx and the interlacing check leaves diff at 0; the first and the
    last row have no such check.  The clamp to d +- 0 returns d."""
    r, c = 9, 33
    slope = np.random.RandomState(5).randint(-12, 13, size=c)
    frame = 100 + slope[None, :] * np.arange(r)[:, None]
    v = np.repeat(frame[None], 3, 0).astype(np.uint8)
    out, counts = deinterlace_matrix(v, order)
    assert np.array_equal(out, np.repeat(v, 2, 0))
    assert counts["widened"] == 0


def test_a_high_depth_sample_above_the_top_reads_as_the_top():
    v = np.full((1, 5, 9), 100, np.uint16)
    v[0, 2, 4] = 60000                                                               # a kept row's sample of field 0: c / e of rows 1 and 3
    w = v.copy()
    w[0, 2, 4] = 1023
    a, b = deinterlace_matrix(v, "tff", 1, 10)[0], deinterlace_matrix(w, "tff", 1, 10)[0]
    assert np.array_equal(a[0, 1::2], b[0, 1::2]) and np.array_equal(a[1], b[1])      # every interpolated sample reads 1023
    assert a[0, 2, 4] == 60000 and b[0, 2, 4] == 1023                                # the kept row is copied as it is
    assert a.max() == 60000 and np.delete(a.reshape(-1), np.argmax(a)).max() <= 1023


@pytest.mark.parametrize("r", [8, 9])
@pytest.mark.parametrize("order", FIELD_ORDERS)
def test_rotating_by_180_degrees_commutes(order, r):
    """rot180 swaps up and dn, x + j with x - j, b with f: the rule is symmetric under it.  An even R also swaps the row parities, which
    is the other field order."""
    other = order if r % 2 else FIELD_ORDERS[1 - FIELD_ORDERS.index(order)]
    for step in STEPS:
        for name, v in input_set(r, 33 * step, step):
            rot = np.ascontiguousarray(v[:, ::-1, ::-1])
            if step > 1:                                                           # (pixels reversed, the channels of a pixel kept in order)
                rot = np.ascontiguousarray(v.reshape(N_FRAMES, r, 33, step)[:, ::-1, ::-1]).reshape(N_FRAMES, r, 33 * step)
            want = deinterlace_matrix(v, order, step)[0]
            want = want[:, ::-1, ::-1] if step == 1 else want.reshape(-1, r, 33, step)[:, ::-1, ::-1].reshape(-1, r, 33 * step)
            assert np.array_equal(deinterlace_matrix(rot, other, step)[0], want), (name, order, r, step)


def test_every_branch_is_taken_by_the_shared_inputs():
    """The guard: the inputs the GPU tests run reach every branch of the rule, in both orders, at 9 x 33 pixels (the one-sample form's
    shape) and 9 x 48 pixels (the vector form's), with steps 1 to 4 and at 10 and 12 bits."""
    cases = [(33, 1, 255, 8), (33, 3, 255, 8), (33, 1, 1023, 10)] + [(48, s, 255, 8) for s in (1, 2, 3, 4)] + [(48, 1, 1023, 10), (48, 1, 4095, 12)]
    for order in FIELD_ORDERS:
        for px, step, top, depth in cases:
            total = dict.fromkeys(BRANCHES, 0)
            per_input = {}
            for name, v in input_set(9, px * step, step, top):
                counts = deinterlace_matrix(v, order, step, depth)[1]
                per_input[name] = counts
                for k in BRANCHES:
                    total[k] += counts[k]
            assert all(total[k] > 0 for k in BRANCHES), (order, px, step, depth, total)
            assert all(per_input["diagonals"][k] > 0 for k in BRANCHES[:4]), per_input["diagonals"]          # +-1 and +-2 win there
            assert per_input["static"]["clamp_lo"] + per_input["static"]["clamp_hi"] > 0


# ---------------------------------------------------------------------------------------------------------------------- frames
def test_packed_frames_are_their_channels_planes():
    """Step c: a channel only meets itself."""
    v = np.random.RandomState(6).randint(0, 256, size=(3, 9, 11, 3)).astype(np.uint8)
    out = deinterlace_frames(v, "bff")
    assert out.shape == (6, 9, 11, 3) and out.dtype == np.uint8
    for k in range(3):
        assert np.array_equal(out[..., k], deinterlace_matrix(v[..., k], "bff")[0])
    assert np.array_equal(deinterlace_frames(torch.from_numpy(v), "bff"), out)


@pytest.mark.parametrize("layout,depth", [("420", 8), ("422", 8), ("444", 10), ("420", 12), ("400", 8), ("400", 10)])
def test_planar_frames_are_deinterlaced_plane_by_plane(layout, depth):
    h, w = 7, 10
    fmt = "y400" if layout == "400" else yuv.FORMAT_OF[layout]
    fb = yuv.frame_bytes(h, w, depth, layout)
    rng = np.random.RandomState(7)
    if depth == 8:
        frames = rng.randint(0, 256, size=(3, fb), dtype=np.uint8)
    else:
        frames = rng.randint(0, 1 << depth, size=(3, fb // 2)).astype("<u2").view(np.uint8).reshape(3, fb)
    out, counts = deinterlace_frames_counted(frames, "tff", fmt, (h, w), depth)
    assert out.shape == (6, fb) and out.dtype == np.uint8
    planes = [yuv.luma_plane(frames, h, w, depth, layout)] if layout == "400" else yuv.split_planes(frames, h, w, depth, layout)
    got = [yuv.luma_plane(out, h, w, depth, layout)] if layout == "400" else yuv.split_planes(out, h, w, depth, layout)
    total = 0
    for p, g in zip(planes, got):
        want, cnt = deinterlace_matrix(p, "tff", 1, depth)
        assert np.array_equal(g, want), (layout, depth)
        total += cnt["clamp_lo"]
    assert counts["clamp_lo"] == total


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    v = np.zeros((2, 4, 6), np.uint8)
    with pytest.raises(ValueError, match="one of tff, bff"):
        deinterlace_matrix(v, "top")
    with pytest.raises(ValueError, match="one of tff, bff"):
        check_order(None)
    with pytest.raises(ValueError, match="R = 1"):
        deinterlace_matrix(np.zeros((2, 1, 6), np.uint8), "tff")
    with pytest.raises(ValueError, match="no frames"):
        deinterlace_matrix(np.zeros((0, 4, 6), np.uint8), "tff")
    with pytest.raises(ValueError, match="integers"):
        deinterlace_matrix(np.zeros((2, 4, 6), np.float32), "tff")
    for step in (0, 5, 4, True):                                                     # (4 does not divide 6)
        with pytest.raises(ValueError, match="step"):
            deinterlace_matrix(v, "tff", step)
    with pytest.raises(ValueError, match="depth"):
        deinterlace_matrix(v, "tff", 1, 9)
    with pytest.raises(ValueError, match="float frames have no integer samples"):
        deinterlace_frames(np.zeros((2, 3, 4, 6), np.float32), "tff")
    with pytest.raises(ValueError, match="one row"):
        deinterlace_frames(np.zeros((2, 1, 6, 3), np.uint8), "tff")
    with pytest.raises(ValueError, match="h >= 3"):
        deinterlace_frames(np.zeros((2, yuv.frame_bytes(2, 4)), np.uint8), "tff", "i420", (2, 4))
    assert deinterlace_frames(np.zeros((2, yuv.frame_bytes(2, 4, 8, "422")), np.uint8), "tff", "i422", (2, 4)).shape == (4, 16)
    with pytest.raises(ValueError, match=r"are \[N, 36\] uint8"):
        deinterlace_frames(np.zeros((2, 35), np.uint8), "tff", "i420", (4, 6))
    with pytest.raises(ValueError, match="needs size"):
        deinterlace_frames(np.zeros((2, 36), np.uint8), "tff", "i420")
    with pytest.raises(ValueError, match="depth = 10 goes with"):
        deinterlace_frames(np.zeros((2, 4, 6, 3), np.uint8), "tff", depth=10)
    with pytest.raises(ValueError, match="channels"):
        deinterlace_frames(np.zeros((2, 4, 6, 5), np.uint8), "tff")


def test_the_public_calls_refuse_before_the_gpu_is_needed():
    import savsr_amd
    from savsr_amd.video import VideoUpscaler, _check_fields
    assert callable(savsr_amd.deinterlace) and savsr_amd.deinterlace.deinterlace_matrix is deinterlace_matrix
    with pytest.raises(ValueError, match="one of tff, bff"):
        savsr_amd.deinterlace(torch.zeros(2, 4, 6, 3, dtype=torch.uint8), "progressive")
    with pytest.raises(ValueError, match="float frames have no integer samples"):
        savsr_amd.deinterlace(torch.zeros(2, 3, 4, 6), "tff")
    with pytest.raises(ValueError, match="one row"):
        savsr_amd.deinterlace(torch.zeros(2, 1, 6, 3, dtype=torch.uint8), "tff")
    with pytest.raises(ValueError, match="h >= 3"):
        savsr_amd.deinterlace(torch.zeros(2, yuv.frame_bytes(2, 4), dtype=torch.uint8), "tff", "i420", (2, 4))
    with pytest.raises(ValueError, match="fields = 'top': one of tff, bff"):
        _check_fields("top")
    assert _check_fields(None) is None and _check_fields("bff") == "bff"
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR().eval()
    with pytest.raises(ValueError, match="fields = 'auto': one of tff, bff"):
        net.upscale_video(torch.zeros(8, 4, 6, 3, dtype=torch.uint8), fields="auto")
    with pytest.raises(ValueError, match="float frames have no integer samples"):
        VideoUpscaler(net, 2, fields="tff").push(torch.zeros(2, 3, 4, 6))
    with pytest.raises(ValueError, match="too few"):                               # check_length applies to 2N: 2 x 1 frames, a 7-frame window
        net.upscale_video(torch.zeros(1, 4, 6, 3, dtype=torch.uint8), fields="tff")


def test_the_module_is_callable_and_survives_reload_and_pickle():
    """savsr_amd.deinterlace is this module and, called, the GPU function (the issue names both); the module's class is swapped for that.
    importlib.reload re-executes the module and keeps it callable; its functions pickle by reference as any module's do."""
    import importlib
    import pickle
    import sys
    import savsr_amd
    mod = savsr_amd.deinterlace
    assert mod is sys.modules["savsr_amd.deinterlace"] and callable(mod) and mod.__name__ == "savsr_amd.deinterlace"
    again = importlib.reload(mod)
    assert again is mod and callable(mod) and savsr_amd.deinterlace is mod
    assert pickle.loads(pickle.dumps(mod.deinterlace_matrix)) is mod.deinterlace_matrix
    assert pickle.loads(pickle.dumps(mod.resolve_fields))("auto", "b", (25, 1))[0] == "bff"
    v = np.random.RandomState(1).randint(0, 256, size=(2, 5, 9)).astype(np.uint8)
    assert np.array_equal(mod.deinterlace_matrix(v, "tff")[0], scalar_deinterlace(v, "tff"))


# ---------------------------------------------------------------------------------------------------------------------- the CLI's header
def test_resolve_fields():
    fps = (30000, 1001)
    # the default and "progressive": everything passes through; a note only when the flag was not given and the tag says interlaced
    for tag in ("p", "t", "b", "m", "?"):
        order, out_tag, out_fps, note = resolve_fields(None, tag, fps)
        assert (order, out_tag, out_fps) == (None, tag, fps)
        assert (note is not None) == (tag in "tbm")
        if note:
            assert "treated as progressive" in note and "--fields" in note and f"I{tag}" in note
        assert resolve_fields("progressive", tag, fps) == (None, tag, fps, None)
    assert resolve_fields(None, None, (25, 1)) == (None, "p", (25, 1), None)         # a PNG folder
    assert resolve_fields("auto", "t", fps) == ("tff", "p", (60000, 1001), None)
    assert resolve_fields("auto", "b", (25, 1)) == ("bff", "p", (50, 1), None)
    assert resolve_fields("auto", "p", (25, 1)) == (None, "p", (25, 1), None)
    with pytest.raises(ValueError, match="Im"):
        resolve_fields("auto", "m", fps)
    with pytest.raises(ValueError, match="PNG folder"):
        resolve_fields("auto", None, fps)
    for flag in FIELD_ORDERS:
        for tag in ("p", "t", "b", "m", None):                                       # an explicit order overrides the tag
            assert resolve_fields(flag, tag, (25, 1)) == (flag, "p", (50, 1), None)
    with pytest.raises(ValueError, match="one of progressive, auto, tff, bff"):
        resolve_fields("top", "t", fps)


def test_cli_arguments(tmp_path, capsys):
    from savsr_amd.upscale import parse_args
    base = ["-o", str(tmp_path / "out"), "--scale", "2", "--checkpoint", "net.pth"]
    assert parse_args(["-i", "in.y4m"] + base).fields is None
    assert parse_args(["-i", "in.y4m", "--fields", "auto"] + base).fields == "auto"
    assert parse_args(["-i", str(tmp_path), "--fields", "bff"] + base).fields == "bff"
    with pytest.raises(SystemExit):
        parse_args(["-i", str(tmp_path), "--fields", "auto"] + base)
    assert "PNG folder" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(["-i", "in.y4m", "--fields", "top"] + base)
