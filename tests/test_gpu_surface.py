"""Video surfaces on the GPU: savsr_video_unpack_surface / savsr_video_pack_surface (csrc/surface.hip) against the numpy specification
(savsr_amd/surface.py) bit for bit, what they may touch, and the surface= / out_surface= arguments of upscale_video and VideoUpscaler
as the compositions the README states."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import savsr_amd
from savsr_amd import surface as S
from savsr_amd import yuv
from savsr_amd.surface import Surface
from savsr_amd.utils import synth
from tests import surface_cases as SC
from tests.video_cases import WEIGHT_SEED

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
CANARY = 64


def _lib():
    from savsr_amd import _lib as L
    return L.load()


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(DEV)


def _args(case):
    return case.surface, case.pixel_format, (case.h, case.w), case.depth


def _entry(name, case, src: torch.Tensor, n: int, src_stride: int, dst: torch.Tensor, dst_stride: int, *tail):
    """One of the two entries through the binding, on raw device pointers."""
    lib = _lib()
    tab = case.table
    desc = S.descriptor(tab)
    rc = getattr(lib, name)(src.data_ptr(), n, src_stride, case.h, case.w, case.depth, S.LAYOUTS.index(case.layout), int(tab.msb),
                            desc.ctypes.data_as(C.POINTER(C.c_int64)), len(tab.planes), dst.data_ptr(), dst_stride, *tail,
                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.savsr_last_error()
    torch.cuda.synchronize()


# SAVSR needs h, w >= 2 at the public calls, which every case has
@pytest.mark.parametrize("kind", S.KINDS)
def test_unpack_and_pack_equal_the_specification(kind):
    for case in SC.BY_KIND[kind]:
        surf, planar, packed = SC.surface_frames(case), SC.planar_frames(case), SC.packed_frames(case)
        for put in (_dev, lambda a: torch.from_numpy(np.array(a))):          # GPU and host input
            got = savsr_amd.unpack_surface(put(surf), *_args(case))
            assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), planar), case.id
            got = savsr_amd.pack_surface(put(planar), *_args(case))
            assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), packed), case.id


@pytest.mark.parametrize("kind", S.KINDS)
def test_pack_writes_its_frames_resolved_bytes_and_nothing_else(kind):
    """The destination is prefilled with 0xA5 between two canaries: inside a frame's resolved bytes every byte is the specification's (0
    where no sample maps), the bytes between frames and the canaries stay."""
    for case in SC.BY_KIND[kind]:
        n, stride, nbytes = SC.N_FRAMES, case.stride, case.table.bytes
        raw = torch.full((2 * CANARY + (n - 1) * stride + nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
        raw[:CANARY] = 0x5C
        raw[-CANARY:] = 0x5C
        planar = _dev(SC.planar_frames(case))
        _entry("savsr_video_pack_surface", case, planar, n, planar.shape[1], raw[CANARY:], stride, nbytes)
        got = raw.cpu().numpy()
        assert np.all(got[:CANARY] == 0x5C) and np.all(got[-CANARY:] == 0x5C), case.id
        want = np.full((n, stride), 0xA5, dtype=np.uint8)
        want[:, :nbytes] = SC.packed_frames(case)
        body = got[CANARY:-CANARY]
        assert np.array_equal(body, want.reshape(-1)[:body.size]), case.id
        mask = SC.sample_mask(case)
        assert not np.any(body[:nbytes] & ~mask), case.id          # every uncovered byte (and bit) inside the frame reads 0


@pytest.mark.parametrize("kind", S.KINDS)
def test_unpack_reads_no_byte_that_holds_no_sample(kind):
    """The source is a view that ends exactly at the last valid byte of the last frame's last row, inside a larger poisoned allocation:
    the result does not change when the poison (the allocation around the view, and every bit inside it that carries no sample) does."""
    for case in SC.BY_KIND[kind]:
        n, stride, span = SC.N_FRAMES, case.stride, case.table.span
        used = (n - 1) * stride + span
        fb = yuv.frame_bytes(case.h, case.w, case.depth, case.layout)
        res = []
        for poison in (0, 1):
            raw = torch.from_numpy(np.random.default_rng(poison).integers(0, 256, 256 + used + 4096, dtype=np.uint8)).to(DEV)
            view = raw[256:256 + used]
            view[:] = _dev(SC.surface_frames(case, poison).reshape(-1)[:used])
            out = torch.full((n * fb + 2 * CANARY,), 0x5C, dtype=torch.uint8, device=DEV)
            _entry("savsr_video_unpack_surface", case, view, n, stride, out[CANARY:], fb)
            got = out.cpu().numpy()
            assert np.all(got[:CANARY] == 0x5C) and np.all(got[-CANARY:] == 0x5C), case.id
            res.append(got[CANARY:-CANARY])
        assert np.array_equal(res[0], res[1]) and np.array_equal(res[0], SC.planar_frames(case).reshape(-1)), case.id


@pytest.mark.parametrize("kind", S.KINDS)
def test_vector_and_sample_forms_give_equal_bytes(kind):
    """The same frames at pitch 128 from an aligned base pointer (the vector form) and at an odd storage offset of a uint8 view (a sample
    per access; a 2-byte offset with 16-bit samples, which must stay aligned to their words)."""
    for case in SC.BY_KIND[kind]:
        if case.pitch != "vector":
            continue
        surf, planar = SC.surface_frames(case), SC.planar_frames(case)
        n, stride = surf.shape
        off = 1 if case.depth == 8 else 2
        aligned = _dev(surf)
        assert aligned.data_ptr() % 16 == 0 and stride % 16 == 0 and all(p.offset % 16 == 0 and p.pitch % 16 == 0 for p in case.table.planes)
        shifted = torch.zeros(n * stride + 16, dtype=torch.uint8, device=DEV)[off:off + n * stride].view(n, stride)
        shifted[:] = aligned
        assert shifted.data_ptr() % 16 == off
        a = savsr_amd.unpack_surface(aligned, *_args(case))
        b = savsr_amd.unpack_surface(shifted, *_args(case))
        assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), planar), case.id
        # pack: the destination of the entry aligned, and off the grid
        out = []
        for o in (0, off):
            raw = torch.full((n * stride + 16,), 0xA5, dtype=torch.uint8, device=DEV)
            _entry("savsr_video_pack_surface", case, _dev(planar), n, planar.shape[1], raw[o:], stride, case.table.bytes)
            out.append(raw[o:o + n * stride].cpu().numpy())
        assert np.array_equal(out[0], out[1]), case.id


def test_entries_refuse_bad_arguments_before_the_device():
    lib = _lib()
    case = next(c for c in SC.BY_KIND["nv12"] if c.pitch == "aligned" and c.w == 34)
    tab = case.table
    src, dst = _dev(SC.surface_frames(case)), torch.zeros(3, 306, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(desc=None, n=3, stride=case.stride, h=case.h, w=case.w, depth=8, chroma=0, msb=0, planes=2, pstride=306, srcp=None):
        d = S.descriptor(tab) if desc is None else desc
        rc = lib.savsr_video_unpack_surface(src.data_ptr() if srcp is None else srcp, n, stride, h, w, depth, chroma, msb,
                                            d.ctypes.data_as(C.POINTER(C.c_int64)), planes, dst.data_ptr(), pstride, st)
        return rc, lib.savsr_last_error().decode()

    assert call()[0] == 0

    def changed(plane, word, value):
        d = S.descriptor(tab)
        d[plane, word] = value
        return d

    for kw, why in ((dict(srcp=0), "null pointer"), (dict(n=0), "n_frames >= 1"), (dict(h=0), "h, w in 1"), (dict(depth=9), "depth 8, 10 or 12"),
                    (dict(chroma=4), "chroma 0"), (dict(msb=1), "msb 0 or 1, and 1 at depth 10 / 12 only"), (dict(planes=4), "1 .. 3 surface planes"),
                    (dict(pstride=305), "planar_frame_bytes smaller than a planar frame"),
                    (dict(stride=tab.span - 1), "surface_frame_bytes smaller than a plane's offset plus its rows"),
                    (dict(desc=changed(1, 4, 3)), "step 1, 2 or 4"), (dict(desc=changed(0, 1, 33)), "pitch below the row's bytes"),
                    (dict(desc=changed(0, 0, -16)), "offset >= 0"), (dict(desc=changed(1, 2, 4)), "has the rows of the planar planes it carries"),
                    (dict(desc=changed(1, 3, 18)), "more groups than the planar row has samples"), (dict(desc=changed(1, 5, 3)), "a plane of the layout"),
                    (dict(desc=changed(1, 0, 128)), "surface planes overlap"), (dict(chroma=3), "a plane of the layout")):
        rc, msg = call(**kw)
        assert rc == -1 and why in msg, (kw, msg)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ the public interface
@pytest.fixture(scope="module")
def net3():
    from savsr_amd.archs.savsr_arch import SAVSR
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=WEIGHT_SEED), strict=True)
    return net.to(DEV).eval()


N, H, W, SC2 = 9, 12, 20, 2


def _planar(layout, depth, seed):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 1 << depth, (N, yuv.frame_bytes(H, W, 8, layout)))
    return v.astype("<u2").view(np.uint8).reshape(N, -1) if depth > 8 else v.astype(np.uint8)


def _in_surface(planar, surf, layout, depth, seed, extra=7):
    """The planar frames in `surf`, with random bits wherever no sample lies and a frame stride beyond the surface's bytes."""
    packed = S.pack_frames(planar, surf, H, W, depth, layout)
    mask = S.pack_frames(np.full((1, planar.shape[1]), 255, np.uint8), surf, H, W, depth, layout)
    out = np.random.default_rng(seed).integers(0, 256, (N, packed.shape[1] + extra + (extra % 2 if depth > 8 else 0)), dtype=np.uint8)
    out[:, :packed.shape[1]] = packed | (out[:, :packed.shape[1]] & ~mask)
    return out


END_TO_END = {
    "nv12": dict(layout="420", depth=8, surface=Surface.nv12(pitch=32, lines=16), out="i420", out_surface=Surface.nv12(pitch_align=64, lines_align=16), kw={}),
    "p010": dict(layout="420", depth=10, surface=Surface.p010(pitch_align=64), out="i420", out_surface=Surface.p010(pitch_align=256), kw=dict(out_depth=10)),
    "uyvy_fields": dict(layout="422", depth=8, surface=Surface.uyvy(pitch=48), out="i420", out_surface=None, kw=dict(fields="tff")),
    "planar_crop": dict(layout="420", depth=8, surface=Surface.planar(pitch=32, lines=13), out="i420", out_surface=Surface.nv12(pitch=48),
                        kw=dict(crop=(2, 4, 8, 12), bars="keep")),
}


@pytest.mark.parametrize("name", list(END_TO_END))
def test_upscale_video_with_surfaces_is_the_composition(net3, name):
    """Property 1: upscale_video(f, surface=s) is upscale_video(unpack_surface(f, s)); property 2: upscale_video(out_surface=t) is
    pack_surface(upscale_video(...), t) at the output's size and depth.  Bit for bit."""
    c = END_TO_END[name]
    fmt = SC.FORMAT_OF[c["layout"]]
    planar = _planar(c["layout"], c["depth"], seed=len(name))
    frames = torch.from_numpy(_in_surface(planar, c["surface"], c["layout"], c["depth"], seed=3))
    common = dict(scale=SC2, pixel_format=fmt, size=(H, W), depth=c["depth"], out=c["out"], **c["kw"])
    unpacked = savsr_amd.unpack_surface(frames, c["surface"], fmt, (H, W), c["depth"])
    assert np.array_equal(unpacked.cpu().numpy(), planar)
    ref = net3.upscale_video(unpacked, **common)                                   # planar in, planar out: the path as it was
    n_out = 2 * N if "fields" in c["kw"] else N
    od = c["kw"].get("out_depth", c["depth"])
    assert ref.shape == (n_out, yuv.frame_bytes(SC2 * H, SC2 * W, od, "420"))
    got = net3.upscale_video(frames, surface=c["surface"], **common)               # property 1, host frames
    assert torch.equal(got, ref)
    got = net3.upscale_video(frames.to(DEV), surface=c["surface"], **common)       # ... and resident ones
    assert torch.equal(got, ref)
    if c["out_surface"] is not None:                                               # property 2, alone and with property 1
        want = savsr_amd.pack_surface(ref, c["out_surface"], c["out"], (SC2 * H, SC2 * W), od)
        assert np.array_equal(want.cpu().numpy(), S.pack_frames(ref.cpu().numpy(), c["out_surface"], SC2 * H, SC2 * W, od, "420"))
        assert torch.equal(net3.upscale_video(unpacked, out_surface=c["out_surface"], **common), want)
        assert torch.equal(net3.upscale_video(frames, surface=c["surface"], out_surface=c["out_surface"], **common), want)


def test_bars_drop_packs_the_picture_alone(net3):
    c = END_TO_END["planar_crop"]
    planar = torch.from_numpy(_planar("420", 8, seed=2))
    kw = dict(scale=SC2, pixel_format="i420", size=(H, W), out="i420", crop=(2, 4, 8, 12), bars="drop")
    ref = net3.upscale_video(planar, **kw)
    got = net3.upscale_video(planar, out_surface=c["out_surface"], **kw)
    assert torch.equal(got, savsr_amd.pack_surface(ref, c["out_surface"], "i420", (16, 24)))


def test_video_upscaler_with_surfaces_any_chunking_is_bitwise(net3):
    from savsr_amd import VideoUpscaler
    c = END_TO_END["nv12"]
    frames = torch.from_numpy(_in_surface(_planar("420", 8, seed=11), c["surface"], "420", 8, seed=4))
    kw = dict(pixel_format="i420", size=(H, W), out="i420", surface=c["surface"], out_surface=c["out_surface"])
    whole = net3.upscale_video(frames, scale=SC2, **kw)
    for chunk in (4, N):
        up = VideoUpscaler(net3, SC2, **kw)
        parts = [up.push(frames[a:a + chunk] if chunk != 4 or a else frames[a:a + chunk].to(DEV)) for a in range(0, N, chunk)] + [up.finish()]
        assert all(p.dtype == torch.uint8 and p.shape[1] == whole.shape[1] for p in parts)
        assert torch.equal(torch.cat(parts, 0), whole), chunk
    # with a stage in front that holds frames back, and a crop: the first push returns no frame, packed as such
    c = END_TO_END["uyvy_fields"]
    frames = torch.from_numpy(_in_surface(_planar("422", 8, seed=12), c["surface"], "422", 8, seed=5))
    kw = dict(pixel_format="i422", size=(H, W), out="i420", surface=c["surface"], out_surface=Surface.nv12(pitch=64), fields="tff",
              crop=(2, 4, 8, 12), bars="keep")
    whole = net3.upscale_video(frames, scale=SC2, **kw)
    up = VideoUpscaler(net3, SC2, **kw)
    parts = [up.push(frames[a:a + 4]) for a in range(0, N, 4)] + [up.finish()]
    assert torch.equal(torch.cat(parts, 0), whole) and whole.shape == (2 * N, 64 * 36)


def test_defaults_run_the_path_as_it_was(net3):
    """With neither argument the call is the planar path: on the frames of tests/golden/yuv_outputs.npz it equals the fp32 path on the
    specification's conversion of them (tests/test_gpu_yuv.py's property), and a tight planar Surface, the identity, changes nothing."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "yuv_outputs.npz"))
    h, w = 8, 10
    frames = gold[f"in/{h}x{w}/i420"]
    assert float(np.abs(yuv.i420_to_rgb(frames, h, w).astype(np.float64) - gold[f"in/{h}x{w}/rgb"]).max()) <= 2e-6
    kw = dict(scale=SC2, padding="replicate")
    ref = net3.upscale_video(torch.from_numpy(yuv.i420_to_rgb(frames, h, w)).to(DEV), **kw)
    got = net3.upscale_video(torch.from_numpy(frames), pixel_format="i420", size=(h, w), **kw)
    assert torch.equal(got, ref)
    q = net3.upscale_video(torch.from_numpy(frames), pixel_format="i420", size=(h, w), out="i420", **kw)
    assert np.array_equal(q.cpu().numpy(), yuv.rgb_to_i420(ref.cpu().numpy()))
    same = net3.upscale_video(torch.from_numpy(frames), pixel_format="i420", size=(h, w), out="i420", surface=Surface.planar(),
                              out_surface=Surface.planar(), **kw)
    assert torch.equal(same, q)


def test_entries_are_capturable():
    case = next(c for c in SC.BY_KIND["p010"] if c.pitch == "vector" and c.w == 66)
    surf, planar = _dev(SC.surface_frames(case)), _dev(SC.planar_frames(case))
    out_p, out_s = torch.zeros_like(planar), torch.full((SC.N_FRAMES, case.table.bytes), 0xA5, dtype=torch.uint8, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            _entry_nosync("savsr_video_unpack_surface", case, surf, SC.N_FRAMES, case.stride, out_p, planar.shape[1])
            _entry_nosync("savsr_video_pack_surface", case, out_p, SC.N_FRAMES, planar.shape[1], out_s, case.table.bytes, case.table.bytes)
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_p, planar) and np.array_equal(out_s.cpu().numpy(), SC.packed_frames(case))


def _entry_nosync(name, case, src, n, src_stride, dst, dst_stride, *tail):
    lib = _lib()
    desc = S.descriptor(case.table)
    rc = getattr(lib, name)(src.data_ptr(), n, src_stride, case.h, case.w, case.depth, S.LAYOUTS.index(case.layout), int(case.table.msb),
                            desc.ctypes.data_as(C.POINTER(C.c_int64)), len(case.table.planes), dst.data_ptr(), dst_stride, *tail,
                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.savsr_last_error()
