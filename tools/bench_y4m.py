"""Raw YUV 4:2:0 in and out, measured.  Every leg is a process of its own under its own time limit; a leg that
fails, times out or dies ends the run (nothing more is started on the GPU) and what the earlier legs gave is kept.

  kernels   savsr_video_gather_i420 / _quantize_i420 beside savsr_video_gather_u8 / _quantize_u8 of the same build, in one process,
            interleaved rounds, at 180x320 and 720x1280: us, the fraction of 8 TB/s on 4*3*h*w + 1.5*h*w bytes, and the ratio to the RGB
            kernel's time (they move the same fp32 bytes and half the uint8 bytes; 1.2x is allowed for the two-row coupling); and
            savsr_video_gather_yuv420 / _quantize_yuv420 with each of the four colour ids (id 0 is the kernel of the _i420 entries)
  depth     savsr_video_gather_yuv420_16 / _quantize_yuv420_16 (10 and 12 bits) beside the 8-bit savsr_video_gather_yuv420 /
            _quantize_yuv420 of the same build, in one process, interleaved rounds, at 180x320 and 720x1280: us, the fraction of 8 TB/s
            on 4*3*h*w + 3*h*w bytes, and the ratio to the 8-bit kernel's time beside the ratio of the bytes moved, (12 + 3) / (12 + 1.5)
            = 1.11 -- a measured ratio well above it means the 16-bit access pattern is wrong.  No time is fixed in advance.
            `--legs depth --out profiles/bench_y4m_depth.json`
  chroma    savsr_video_gather_yuvp / _quantize_yuvp at 4:2:2 and 4:4:4 beside the 4:2:0 kernels of the same build (chroma = 0 of the same
            entries), at 8 and 10 bits, in one process, interleaved rounds, at 720x1280: us, bytes in and out, GB/s = (bytes in + bytes
            out) / time.  The layouts move different bytes per pixel, so the GB/s are compared, not the times; the 4:2:0 kernels are
            timed twice in every round and the spread between their two readings is the margin (`margin_gbs`).  No time is fixed in
            advance.  `--legs chroma --out profiles/bench_y4m_chroma.json`
  siting    savsr_video_gather_yuvs / _quantize_yuvs (linear chroma reconstruction in, cosited filters out) at every siting of 4:2:0 and
            4:2:2 beside that layout's nearest / box kernel (siting 0 of the same entries), at 8 and 10 bits, 720x1280, 7 frames, in one
            process, interleaved rounds: us, bytes in and out, GB/s.  The nearest kernel is timed twice in every round and the spread
            between its two readings is the margin.  The same leg computes on the CPU, from yuv.py alone, what the feature is worth on a
            synthetic picture (`value_psnr`): smooth seeded fields plus chroma edges, subsampled by a float64 left-cosited [1 2 1] / 4,
            reconstructed by today's nearest reading and by siting="left"; PSNR of the reconstructed chroma.  Synthetic: no real footage.
            `--legs siting --out profiles/bench_y4m_siting.json`
  luma      savsr_video_gather_luma / _quantize_luma / _resample_chroma (luma-only checkpoints) at 8 and 10 bits, 7 frames, in one process,
            interleaved rounds: the two luma kernels at 720x1280 beside savsr_video_gather_yuvp / _quantize_yuvp at 4:2:0, which are read
            twice in every round (their spread is the margin); the resampler at x4 from 180x320 for 4:2:0 -> 4:2:0 and 4:2:0 -> 4:4:4 (one
            call per plane; the figure is U and V together).  us, bytes in and out, GB/s = (bytes in + bytes out) / time.  No speed is
            fixed in advance.  `--legs luma --out profiles/bench_y4m_luma.json`
  dither    the three quantiser entries with a dither argument (savsr_video_quantize_u8_d, _quantize_yuvs_d at 4:2:0 8-bit and 10-bit,
            _quantize_luma_d at 8 bits) with dither 0 and 1, 7 frames of 720x1280, in one process, interleaved rounds; the dither-0 twin is
            read twice in every round and the spread between its two readings is the margin (`margin_us`).  us, bytes in and out, GB/s,
            and the moved-bytes floor at 8 TB/s beside every reading.  Then upscale_video on config 2's clip (180x320 x4) with
            out="uint8" and out="i420", with and without dither="ordered", interleaved, frames/s.  With --parent CHECKOUT (a checkout of
            the parent commit with its library built) the entries without a dither argument -- savsr_video_quantize_u8, _quantize_yuvs,
            _quantize_luma, which both trees have -- are read in fresh processes, parent / this tree / parent / this tree; the margin is
            the spread between the parent's own processes.  No time is fixed in advance.
            `--legs dither --parent CHECKOUT --out profiles/bench_y4m_dither.json`
  ceiling   upscale_video on preloaded I420 frames, I420 out (frames/s): what the CLI could reach
  cli       python -m savsr_amd.upscale on one synthetic video, PNG folder -> PNG folder against .y4m -> .y4m, A/B/A/B; files under
            --workdir (name the disk it lies on beside the figures: tmpfs or a scratch disk)
  psnr      PSNR-Y of (I420 -> device path -> I420) and of (I420 -> host 8-bit RGB -> the uint8 RGB path -> host 8-bit YUV), each
            against the float result of the I420 input converted in float64.  Synthetic weights: the ranking of the two paths is what
            the figure shows, not a quality claim.

    python3 tools/bench_y4m.py --out profiles/bench_y4m.json [--workdir /dev/shm]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
LEG_TIMEOUT_S = {"dither": 300, "dither_ab": 120, "kernels": 240, "depth": 240, "chroma": 240, "siting": 300, "luma": 240, "ceiling": 420, "cli": 420, "psnr": 420}


def _net(dev):
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.utils import synth
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=0), strict=True)
    return net.to(dev).eval()


def _video_i420(n, h, w):
    """A smooth seeded video in I420 (random bytes are the worst case of no codec; PNG encoding time depends on the content)."""
    import numpy as np
    from savsr_amd import yuv
    from savsr_amd.utils import synth
    clip = synth.synth_clip(n, 3, h, w, seed=3)[0].numpy().astype(np.float32)
    return yuv.rgb_to_i420(clip)


def leg_kernels(a):
    import ctypes as C
    import torch
    from savsr_amd import _lib
    from savsr_amd.yuv import COLOURS, i420_bytes
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for h, w in ((180, 320), (720, 1280)):
        n, idx = 16, list(range(7))
        arr = (C.c_int32 * 7)(*idx)
        rgb8 = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=dev)
        i420 = torch.randint(0, 256, (n, i420_bytes(h, w)), dtype=torch.uint8, device=dev)
        slots = torch.empty(7, 3, h, w, device=dev)
        x = torch.rand(7, 3, h, w, device=dev)
        q8 = torch.empty(7, h, w, 3, dtype=torch.uint8, device=dev)
        q420 = torch.empty(7, i420_bytes(h, w), dtype=torch.uint8, device=dev)
        fns = {
            "savsr_video_gather_u8": lambda: lib.savsr_video_gather_u8(rgb8.data_ptr(), n, 3, h, w, arr, 7, slots.data_ptr(), st),
            "savsr_video_gather_i420": lambda: lib.savsr_video_gather_i420(i420.data_ptr(), n, h, w, arr, 7, slots.data_ptr(), st),
            "savsr_video_quantize_u8": lambda: lib.savsr_video_quantize_u8(x.data_ptr(), 7, 3, h, w, q8.data_ptr(), st),
            "savsr_video_quantize_i420": lambda: lib.savsr_video_quantize_i420(x.data_ptr(), 7, h, w, q420.data_ptr(), st),
        }
        for c, name in enumerate(COLOURS):
            fns[f"savsr_video_gather_yuv420 {name}"] = lambda c=c: lib.savsr_video_gather_yuv420(i420.data_ptr(), n, h, w, arr, 7, c, slots.data_ptr(), st)
            fns[f"savsr_video_quantize_yuv420 {name}"] = lambda c=c: lib.savsr_video_quantize_yuv420(x.data_ptr(), 7, h, w, c, q420.data_ptr(), st)
        us = {k: [] for k in fns}
        for k, fn in fns.items():
            assert fn() == 0, k
        torch.cuda.synchronize()
        for _ in range(a.rounds):                       # interleaved rounds: every kernel sees the same clocks
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us[k].append(1e3 * e0.elapsed_time(e1) / a.iters)
        med = {k: statistics.median(v) for k, v in us.items()}
        for k in fns:
            byte_side = 1.5 if "420" in k else 3.0
            nbytes = 7 * (4 * 3 + byte_side) * h * w
            row = {"kernel": k, "size": [h, w], "frames": 7, "us": round(med[k], 2), "us_per_frame": round(med[k] / 7, 3),
                   "mb": round(nbytes / 1e6, 2), "hbm_frac": round(nbytes / (med[k] * 1e-6) / HBM_BYTES_PER_S, 3)}
            if "420" in k:
                row["vs_rgb_kernel"] = round(med[k] / med[k.split()[0].replace("yuv420", "u8").replace("i420", "u8")], 3)
            row["us_rounds"] = [round(v, 2) for v in us[k]]          # (the spread between the rounds of this run)
            rows.append(row)
    return {"kernels": rows, "rounds": a.rounds, "iters": a.iters, "timing": "HIP events around `iters` back-to-back launches (launch rate included)"}


def leg_depth(a):
    import ctypes as C
    import torch
    from savsr_amd import _lib
    from savsr_amd.yuv import i420_bytes
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for h, w in ((180, 320), (720, 1280)):
        n, idx = 16, list(range(7))
        arr = (C.c_int32 * 7)(*idx)
        f8 = torch.randint(0, 256, (n, i420_bytes(h, w)), dtype=torch.uint8, device=dev)
        f16 = {d: torch.randint(0, 1 << d, (n, i420_bytes(h, w)), dtype=torch.int16, device=dev).view(torch.uint8).view(n, -1) for d in (10, 12)}
        assert all(int(f.shape[1]) == i420_bytes(h, w, d) for d, f in f16.items())
        slots = torch.empty(7, 3, h, w, device=dev)
        x = torch.rand(7, 3, h, w, device=dev)
        q8 = torch.empty(7, i420_bytes(h, w), dtype=torch.uint8, device=dev)
        q16 = torch.empty(7, i420_bytes(h, w, 10), dtype=torch.uint8, device=dev)
        fns = {"savsr_video_gather_yuv420": lambda: lib.savsr_video_gather_yuv420(f8.data_ptr(), n, h, w, arr, 7, 1, slots.data_ptr(), st),
               "savsr_video_quantize_yuv420": lambda: lib.savsr_video_quantize_yuv420(x.data_ptr(), 7, h, w, 1, q8.data_ptr(), st)}
        for d in (10, 12):
            fns[f"savsr_video_gather_yuv420_16 {d}"] = lambda d=d: lib.savsr_video_gather_yuv420_16(f16[d].data_ptr(), n, h, w, arr, 7, 1, d, slots.data_ptr(), st)
            fns[f"savsr_video_quantize_yuv420_16 {d}"] = lambda d=d: lib.savsr_video_quantize_yuv420_16(x.data_ptr(), 7, h, w, 1, d, q16.data_ptr(), st)
        us = {k: [] for k in fns}
        for k, fn in fns.items():
            assert fn() == 0, k
        torch.cuda.synchronize()
        for _ in range(a.rounds):                       # interleaved rounds: every kernel sees the same clocks
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us[k].append(1e3 * e0.elapsed_time(e1) / a.iters)
        med = {k: statistics.median(v) for k, v in us.items()}
        for k in fns:
            high = "_16" in k
            nbytes = 7 * (4 * 3 + (3.0 if high else 1.5)) * h * w
            row = {"kernel": k, "size": [h, w], "frames": 7, "us": round(med[k], 2), "us_per_frame": round(med[k] / 7, 3),
                   "mb": round(nbytes / 1e6, 2), "hbm_frac": round(nbytes / (med[k] * 1e-6) / HBM_BYTES_PER_S, 3)}
            if high:
                row["vs_8bit_kernel"] = round(med[k] / med[k.split()[0][:-3]], 3)
                row["byte_ratio"] = round((12 + 3.0) / (12 + 1.5), 3)
            row["us_rounds"] = [round(v, 2) for v in us[k]]
            rows.append(row)
    return {"kernels": rows, "rounds": a.rounds, "iters": a.iters, "colour": "bt709",
            "timing": "HIP events around `iters` back-to-back launches (launch rate included)"}


def leg_chroma(a):
    import ctypes as C
    import torch
    from savsr_amd import _lib
    from savsr_amd.yuv import CHROMAS, frame_bytes
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    h, w, n = 720, 1280, 16
    arr = (C.c_int32 * 7)(*range(7))
    slots = torch.empty(7, 3, h, w, device=dev)
    x = torch.rand(7, 3, h, w, device=dev)
    fns, nbytes = {}, {}
    keep = []                                       # (the buffers the closures below read and write)
    for depth in (8, 10):
        for cid, chroma in enumerate(CHROMAS):
            fb = frame_bytes(h, w, depth, chroma)
            src = torch.randint(0, 256 if depth == 8 else 4, (n, fb), dtype=torch.uint8, device=dev)      # (in-range samples at either depth)
            dst = torch.empty(7, fb, dtype=torch.uint8, device=dev)
            keep += [src, dst]
            for tag in (("a", "b") if cid == 0 else ("",)):          # the yardstick is read twice in every round
                name = f"{chroma} {depth}-bit" + (f" ({tag})" if tag else "")
                fns[f"gather {name}"] = lambda s_=src, d=depth, c=cid: lib.savsr_video_gather_yuvp(s_.data_ptr(), n, h, w, arr, 7, 1, d, c, slots.data_ptr(), st)
                fns[f"quantize {name}"] = lambda o=dst, d=depth, c=cid: lib.savsr_video_quantize_yuvp(x.data_ptr(), 7, h, w, 1, d, c, o.data_ptr(), st)
                nbytes[f"gather {name}"] = (7 * fb, 7 * 12 * h * w)
                nbytes[f"quantize {name}"] = (7 * 12 * h * w, 7 * fb)
    us = {k: [] for k in fns}
    for k, fn in fns.items():
        assert fn() == 0, k
    torch.cuda.synchronize()
    for _ in range(a.rounds):                           # interleaved rounds: every kernel sees the same clocks
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(1e3 * e0.elapsed_time(e1) / a.iters)
    med = {k: statistics.median(v) for k, v in us.items()}
    gbs = {k: sum(nbytes[k]) / (med[k] * 1e-6) / 1e9 for k in fns}
    rows = []
    for k in fns:
        side, _, depth = k.split()[:3]
        ya, yb = gbs[f"{side} 420 {depth} (a)"], gbs[f"{side} 420 {depth} (b)"]
        row = {"kernel": k, "size": [h, w], "frames": 7, "us": round(med[k], 2), "bytes_in": nbytes[k][0], "bytes_out": nbytes[k][1],
               "gbs": round(gbs[k], 1), "gbs_420": round(min(ya, yb), 1), "margin_gbs": round(abs(ya - yb), 1),
               "below_420_by_more_than_the_margin": bool(gbs[k] < min(ya, yb) - abs(ya - yb)),
               "us_rounds": [round(v, 2) for v in us[k]]}
        rows.append(row)
    return {"kernels": rows, "rounds": a.rounds, "iters": a.iters, "colour": "bt709",
            "timing": "HIP events around `iters` back-to-back launches (launch rate included)"}


def siting_value_psnr(h=360, w=640, seed=11):
    """On the CPU, from yuv.py alone: full-resolution chroma (smooth seeded fields plus vertical, horizontal and diagonal edges), subsampled
    to 4:2:0 as an MPEG-2 / H.264 encoder's input is -- float64 [1 2 1] / 4 at x = 2 cx (left-cosited), the mean of rows 2 cy, 2 cy + 1 --
    and rounded to 8 bits; then reconstructed by nearest replication (siting=None) and by siting="left".  PSNR of the two reconstructions
    against the full-resolution planes, peak 255."""
    import numpy as np
    from savsr_amd import yuv
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = []
    for _ in range(2):
        f = np.full((h, w), 128.0)
        for _ in range(6):                              # smooth fields
            fy, fx, ph, amp = rng.uniform(0.5, 6) / h, rng.uniform(0.5, 6) / w, rng.uniform(0, 2 * np.pi), rng.uniform(4, 14)
            f += amp * np.sin(2 * np.pi * (fy * yy + fx * xx) + ph)
        for _ in range(10):                             # chroma edges: half planes at random angles
            ang, off, step = rng.uniform(0, np.pi), rng.uniform(0.2, 0.8), rng.uniform(-45, 45)
            f += step * ((np.cos(ang) * xx / w + np.sin(ang) * yy / h) > off * (abs(np.cos(ang)) + abs(np.sin(ang))))
        planes.append(np.clip(f, 16, 240))
    ch, cw = yuv.chroma_hw(h, w)
    xs, ys = 2 * np.arange(cw), 2 * np.arange(ch)

    def down(p):
        hr = (p[:, np.maximum(xs - 1, 0)] + 2 * p[:, xs] + p[:, np.minimum(xs + 1, w - 1)]) / 4.0
        return np.rint((hr[ys] + hr[np.minimum(ys + 1, h - 1)]) / 2.0).astype(np.uint8)

    def psnr(rec):
        mse = np.mean([(r.astype(np.float64) - p) ** 2 for r, p in zip(rec, planes)])
        return round(float(10 * np.log10(255.0 ** 2 / mse)), 2)
    sub = [down(p)[None] for p in planes]
    near = psnr([yuv.replicate_chroma(c, h, w)[0] for c in sub])
    out = {"size": [h, w], "seed": seed, "nearest_db": near}
    for siting in yuv.SITINGS:
        out[f"{siting}_db"] = psnr([yuv.interpolate_chroma(c, h, w, "420", siting)[0] for c in sub])
    out["left_minus_nearest_db"] = round(out["left_db"] - near, 2)
    out["note"] = "synthetic picture, chroma planes only, 8-bit 4:2:0 subsampled left-cosited; no real footage"
    return out


def leg_siting(a):
    import ctypes as C
    import torch
    from savsr_amd import _lib
    from savsr_amd.yuv import CHROMAS, SITINGS, frame_bytes
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    h, w, n = 720, 1280, 16
    arr = (C.c_int32 * 7)(*range(7))
    slots = torch.empty(7, 3, h, w, device=dev)
    x = torch.rand(7, 3, h, w, device=dev)
    fns, nbytes = {}, {}
    keep = []                                       # (the buffers the closures below read and write)
    for depth in (8, 10):
        for cid, chroma in enumerate(CHROMAS[:2]):
            fb = frame_bytes(h, w, depth, chroma)
            src = torch.randint(0, 256 if depth == 8 else 4, (n, fb), dtype=torch.uint8, device=dev)      # (in-range samples at either depth)
            dst = torch.empty(7, fb, dtype=torch.uint8, device=dev)
            keep += [src, dst]
            sitings = [(i + 1, s) for i, s in enumerate(SITINGS) if not (chroma == "422" and s == "topleft")]
            # the yardstick (siting 0: the nearest / box kernel) first and last in every round; quantiser siting 1 is the box kernel itself
            for sid, tag in [(0, "nearest (a)")] + sitings + [(0, "nearest (b)")]:
                name = f"{chroma} {depth}-bit {tag}"
                fns[f"gather {name}"] = lambda s_=src, d=depth, c=cid, i=sid: lib.savsr_video_gather_yuvs(s_.data_ptr(), n, h, w, arr, 7, 1, d, c, i,
                                                                                                          slots.data_ptr(), st)
                nbytes[f"gather {name}"] = (7 * fb, 7 * 12 * h * w)
                if sid != 1:
                    fns[f"quantize {name}"] = lambda o=dst, d=depth, c=cid, i=sid: lib.savsr_video_quantize_yuvs(x.data_ptr(), 7, h, w, 1, d, c, i,
                                                                                                                o.data_ptr(), st)
                    nbytes[f"quantize {name}"] = (7 * 12 * h * w, 7 * fb)
    us = {k: [] for k in fns}
    for k, fn in fns.items():
        assert fn() == 0, k
    torch.cuda.synchronize()
    for _ in range(a.rounds):                           # interleaved rounds: every kernel sees the same clocks
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(1e3 * e0.elapsed_time(e1) / a.iters)
    med = {k: statistics.median(v) for k, v in us.items()}
    gbs = {k: sum(nbytes[k]) / (med[k] * 1e-6) / 1e9 for k in fns}
    rows = []
    for k in fns:
        side, chroma, depth = k.split()[:3]
        ya, yb = gbs[f"{side} {chroma} {depth} nearest (a)"], gbs[f"{side} {chroma} {depth} nearest (b)"]
        rows.append({"kernel": k, "size": [h, w], "frames": 7, "us": round(med[k], 2), "bytes_in": nbytes[k][0], "bytes_out": nbytes[k][1],
                     "gbs": round(gbs[k], 1), "gbs_nearest": round(min(ya, yb), 1), "margin_gbs": round(abs(ya - yb), 1),
                     "below_nearest_pct": round(100.0 * (1.0 - gbs[k] / min(ya, yb)), 1),
                     "below_nearest_by_more_than_the_margin": bool(gbs[k] < min(ya, yb) - abs(ya - yb)),
                     "us_rounds": [round(v, 2) for v in us[k]]})
    return {"kernels": rows, "rounds": a.rounds, "iters": a.iters, "colour": "bt709", "value_psnr": siting_value_psnr(),
            "timing": "HIP events around `iters` back-to-back launches (launch rate included)"}


def leg_luma(a):
    import ctypes as C
    import torch
    from savsr_amd import _lib
    from savsr_amd.yuv import chroma_hw, chroma_tables, frame_bytes
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    h, w, n = 720, 1280, 16
    lh, lw = 180, 320
    arr = (C.c_int32 * 7)(*range(7))
    slots3, slots1 = torch.empty(7, 3, h, w, device=dev), torch.empty(7, 1, h, w, device=dev)
    x3, x1 = torch.rand(7, 3, h, w, device=dev), torch.rand(7, 1, h, w, device=dev)
    fns, nbytes, keep = {}, {}, []
    for depth in (8, 10):
        s = 1 if depth == 8 else 2
        fb = frame_bytes(h, w, depth, "420")
        src = torch.randint(0, 256 if depth == 8 else 4, (n, fb), dtype=torch.uint8, device=dev)          # (in-range samples at either depth)
        dst = torch.empty(7, fb, dtype=torch.uint8, device=dev)
        keep += [src, dst]
        for tag in ("a", "b"):                          # the yardstick is read twice in every round
            fns[f"gather yuvp 420 {depth}-bit ({tag})"] = lambda s_=src, d=depth: lib.savsr_video_gather_yuvp(s_.data_ptr(), n, h, w, arr, 7, 1, d, 0, slots3.data_ptr(), st)
            fns[f"quantize yuvp 420 {depth}-bit ({tag})"] = lambda o=dst, d=depth: lib.savsr_video_quantize_yuvp(x3.data_ptr(), 7, h, w, 1, d, 0, o.data_ptr(), st)
            nbytes[f"gather yuvp 420 {depth}-bit ({tag})"] = (7 * fb, 7 * 12 * h * w)
            nbytes[f"quantize yuvp 420 {depth}-bit ({tag})"] = (7 * 12 * h * w, 7 * fb)
        fns[f"gather luma {depth}-bit"] = lambda s_=src, d=depth, fb=fb: lib.savsr_video_gather_luma(s_.data_ptr(), n, fb, h, w, d, arr, 7, slots1.data_ptr(), st)
        fns[f"quantize luma {depth}-bit"] = lambda o=dst, d=depth, fb=fb: lib.savsr_video_quantize_luma(x1.data_ptr(), 7, h, w, d, o.data_ptr(), fb, st)
        nbytes[f"gather luma {depth}-bit"] = (7 * h * w * s, 7 * 4 * h * w)
        nbytes[f"quantize luma {depth}-bit"] = (7 * 4 * h * w, 7 * h * w * s)
        lfb = frame_bytes(lh, lw, depth, "420")
        lsrc = torch.randint(0, 256 if depth == 8 else 4, (7, lfb), dtype=torch.uint8, device=dev)
        keep.append(lsrc)
        ch, cw = chroma_hw(lh, lw, "420")
        for out_chroma in ("420", "444"):
            tabs = [[torch.from_numpy(v).to(dev) for v in t] for t in chroma_tables(lh, lw, h, w, "420", out_chroma)]
            ofb = frame_bytes(h, w, depth, out_chroma)
            cH, cW = chroma_hw(h, w, out_chroma)
            odst = torch.empty(7, ofb, dtype=torch.uint8, device=dev)
            keep += [tabs, odst]

            def resample(s_=lsrc, o=odst, d=depth, s=s, t=tabs, lfb=lfb, ofb=ofb, cH=cH, cW=cW):
                rc = 0
                for plane in range(2):
                    rc |= lib.savsr_video_resample_chroma(s_.data_ptr(), 7, lfb, (lh * lw + plane * ch * cw) * s, ch, cw, d, o.data_ptr(), ofb,
                                                          (h * w + plane * cH * cW) * s, cH, cW, d, t[0][0].data_ptr(), t[0][1].data_ptr(),
                                                          t[0][2].data_ptr(), int(t[0][2].shape[1]), t[1][0].data_ptr(), t[1][1].data_ptr(),
                                                          t[1][2].data_ptr(), int(t[1][2].shape[1]), st)
                return rc
            fns[f"resample 420->{out_chroma} {depth}-bit"] = resample
            nbytes[f"resample 420->{out_chroma} {depth}-bit"] = (7 * 2 * ch * cw * s, 7 * 2 * cH * cW * s)
    us = {k: [] for k in fns}
    for k, fn in fns.items():
        assert fn() == 0, k
    torch.cuda.synchronize()
    for _ in range(a.rounds):                           # interleaved rounds: every kernel sees the same clocks
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(1e3 * e0.elapsed_time(e1) / a.iters)
    med = {k: statistics.median(v) for k, v in us.items()}
    gbs = {k: sum(nbytes[k]) / (med[k] * 1e-6) / 1e9 for k in fns}
    rows = []
    for k in fns:
        side, depth = k.split()[0], [t for t in k.split() if t.endswith("-bit")][0]
        row = {"kernel": k, "frames": 7, "us": round(med[k], 2), "bytes_in": nbytes[k][0], "bytes_out": nbytes[k][1], "gbs": round(gbs[k], 1),
               "us_rounds": [round(v, 2) for v in us[k]]}
        if side != "resample":
            ya, yb = gbs[f"{side} yuvp 420 {depth} (a)"], gbs[f"{side} yuvp 420 {depth} (b)"]
            row.update(size=[h, w], gbs_yuvp_420=round(min(ya, yb), 1), margin_gbs=round(abs(ya - yb), 1),
                       below_yuvp_by_more_than_the_margin=bool(gbs[k] < min(ya, yb) - abs(ya - yb)))
        else:
            row.update(size=[lh, lw], out_size=[h, w], launches=2)
        rows.append(row)
    return {"kernels": rows, "rounds": a.rounds, "iters": a.iters,
            "timing": "HIP events around `iters` back-to-back launches (launch rate included); a resample reading is its two launches, U and V"}


def _time_rounds(torch, fns, rounds, iters):
    """us per launch of every fn, round by round: HIP events around `iters` back-to-back launches, the fns interleaved in every round."""
    us = {k: [] for k in fns}
    for k, fn in fns.items():
        assert fn() == 0, k
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(1e3 * e0.elapsed_time(e1) / iters)
    return us


def leg_dither(a):
    import torch
    from savsr_amd import _lib
    from savsr_amd.yuv import frame_bytes
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    h, w, n = 720, 1280, 7
    x3, x1 = torch.rand(n, 3, h, w, device=dev), torch.rand(n, 1, h, w, device=dev)
    q8 = torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev)
    fb = {d: frame_bytes(h, w, d, "420") for d in (8, 10)}
    q420 = {d: torch.empty(n, fb[d], dtype=torch.uint8, device=dev) for d in (8, 10)}
    entries = {          # name -> (call(dither), bytes in, bytes out)
        "quantize_u8_d": (lambda d: lib.savsr_video_quantize_u8_d(x3.data_ptr(), n, 3, h, w, d, q8.data_ptr(), st), n * 12 * h * w, n * 3 * h * w),
        "quantize_yuvs_d 420 8-bit": (lambda d: lib.savsr_video_quantize_yuvs_d(x3.data_ptr(), n, h, w, 1, 8, 0, 0, d, q420[8].data_ptr(), st),
                                      n * 12 * h * w, n * fb[8]),
        "quantize_yuvs_d 420 10-bit": (lambda d: lib.savsr_video_quantize_yuvs_d(x3.data_ptr(), n, h, w, 1, 10, 0, 0, d, q420[10].data_ptr(), st),
                                       n * 12 * h * w, n * fb[10]),
        "quantize_luma_d 8-bit": (lambda d: lib.savsr_video_quantize_luma_d(x1.data_ptr(), n, h, w, 8, d, q420[8].data_ptr(), fb[8], st),
                                  n * 4 * h * w, n * h * w),
    }
    fns, moved = {}, {}
    for name, (call, bi, bo) in entries.items():
        for tag, d in (("dither 0 (a)", 0), ("dither 1", 1), ("dither 0 (b)", 0)):          # the twin first and last in every round
            fns[f"{name} {tag}"] = lambda call=call, d=d: call(d)
            moved[f"{name} {tag}"] = (bi, bo)
    us = _time_rounds(torch, fns, a.rounds, a.iters)
    med = {k: statistics.median(v) for k, v in us.items()}
    rows = []
    for k in fns:
        name = k[:k.index(" dither ")]
        ta, tb = med[f"{name} dither 0 (a)"], med[f"{name} dither 0 (b)"]
        rows.append({"kernel": k, "size": [h, w], "frames": n, "us": round(med[k], 2), "bytes_in": moved[k][0], "bytes_out": moved[k][1],
                     "gbs": round(sum(moved[k]) / (med[k] * 1e-6) / 1e9, 1), "floor_us_at_8tbs": round(sum(moved[k]) / HBM_BYTES_PER_S * 1e6, 2),
                     "us_twin": round(min(ta, tb), 2), "margin_us": round(abs(ta - tb), 2),
                     "slower_than_twin_by_more_than_the_margin": bool(med[k] > max(ta, tb) + abs(ta - tb)),
                     "us_rounds": [round(v, 2) for v in us[k]]})
    # end to end: config 2's clip
    net = _net(dev)
    sc = (a.scale, a.scale)
    frames = torch.from_numpy(_video_i420(a.frames, a.h, a.w)).to(dev)
    kw = dict(scale=sc, pixel_format="i420", size=(a.h, a.w))
    plan = [(out, d) for out in ("uint8", "i420") for d in (None, "ordered")]
    fps = {f"{out} dither={d}": [] for out, d in plan}
    with torch.no_grad():
        for out, d in plan:
            net.upscale_video(frames[:16], out=out, dither=d, **kw)
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for out, d in plan:
                t0 = time.perf_counter()
                r = net.upscale_video(frames, out=out, dither=d, **kw)
                torch.cuda.synchronize()
                fps[f"{out} dither={d}"].append(round(a.frames / (time.perf_counter() - t0), 2))
                del r
    return {"kernels": rows, "rounds": a.rounds, "iters": a.iters, "colour": "bt709",
            "timing": "HIP events around `iters` back-to-back launches (launch rate included)",
            "e2e": {"workload": f"{a.frames} frames {a.h}x{a.w} x{a.scale:g}, I420 in", "fps": fps,
                    "fps_median": {k: statistics.median(v) for k, v in fps.items()}}}


def leg_dither_ab(a):
    """The quantiser entries both trees have, on the tree at --root: one fresh process of the parent / this tree comparison."""
    root = os.path.abspath(a.root or ROOT)
    sys.path.insert(0, root)
    import torch
    from savsr_amd import _lib
    from savsr_amd.yuv import frame_bytes
    lib = _lib.load()
    assert os.path.samefile(os.path.dirname(os.path.dirname(_lib.LIB_PATH)), os.path.join(root, "savsr_amd")), _lib.LIB_PATH
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    h, w, n = 720, 1280, 7
    x3, x1 = torch.rand(n, 3, h, w, device=dev), torch.rand(n, 1, h, w, device=dev)
    q8 = torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev)
    fb = frame_bytes(h, w, 8, "420")
    q420 = torch.empty(n, fb, dtype=torch.uint8, device=dev)
    fns = {"savsr_video_quantize_u8": lambda: lib.savsr_video_quantize_u8(x3.data_ptr(), n, 3, h, w, q8.data_ptr(), st),
           "savsr_video_quantize_yuvs 420 8-bit": lambda: lib.savsr_video_quantize_yuvs(x3.data_ptr(), n, h, w, 1, 8, 0, 0, q420.data_ptr(), st),
           "savsr_video_quantize_yuvs 420 8-bit left": lambda: lib.savsr_video_quantize_yuvs(x3.data_ptr(), n, h, w, 1, 8, 0, 2, q420.data_ptr(), st),
           "savsr_video_quantize_luma 8-bit": lambda: lib.savsr_video_quantize_luma(x1.data_ptr(), n, h, w, 8, q420.data_ptr(), fb, st)}
    us = _time_rounds(torch, fns, a.rounds, a.iters)
    return {"tree": "this" if os.path.samefile(root, ROOT) else "parent", "abi": int(lib.savsr_abi_version()),
            "us": {k: round(statistics.median(v), 2) for k, v in us.items()}, "us_rounds": {k: [round(x, 2) for x in v] for k, v in us.items()}}


def dither_parent_ab(a, run_child):
    """parent / this / parent / this in fresh processes; the margin of every kernel is the spread between the parent's own processes."""
    runs = {"parent": [], "this": []}
    for _ in range(a.ab_rounds):
        for tree, root in (("parent", a.parent), ("this", ROOT)):
            r = run_child("dither_ab", ["--root", os.path.abspath(root)])
            if r is None:
                return {"runs": runs, "error": f"the {tree} process failed"}, 1
            runs[tree].append(r)
    out = {"runs": runs, "order": "fresh processes, parent / this tree, round after round", "kernels": {}}
    for k in runs["parent"][0]["us"]:
        pa, th = [r["us"][k] for r in runs["parent"]], [r["us"][k] for r in runs["this"]]
        spread = max(pa) - min(pa)
        out["kernels"][k] = {"parent_us": pa, "this_us": th, "parent_spread_us": round(spread, 2),
                             "this_median_vs_parent_median": round(statistics.median(th) / statistics.median(pa), 4),
                             "this_within_the_parents_range_widened_by_its_spread": bool(statistics.median(th) <= max(pa) + spread)}
    return out, 0


def leg_ceiling(a):
    import torch
    dev = torch.device("cuda:0")
    net = _net(dev)
    sc = (a.scale, a.scale)
    frames = torch.from_numpy(_video_i420(a.frames, a.h, a.w)).to(dev)
    ts = []
    with torch.no_grad():
        net.upscale_video(frames, scale=sc, out="i420", pixel_format="i420", size=(a.h, a.w))
        torch.cuda.synchronize()
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = net.upscale_video(frames, scale=sc, out="i420", pixel_format="i420", size=(a.h, a.w))
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            del r
    return {"ceiling_fps": round(a.frames / statistics.median(ts), 2), "ceiling_fps_all": [round(a.frames / t, 2) for t in ts]}


def leg_cli(a):
    """No GPU in this process: it prepares the files and runs the CLI, one child at a time."""
    import numpy as np
    from PIL import Image
    from savsr_amd import io as sio, y4m, yuv
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.utils import synth
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=0), strict=True)
    frames = _video_i420(a.frames, a.h, a.w)
    rgb8 = np.rint(yuv.i420_to_rgb(frames, a.h, a.w) * np.float32(255.0)).astype(np.uint8).transpose(0, 2, 3, 1)
    res = {"png_fps": [], "y4m_fps": [], "workdir": a.workdir or tempfile.gettempdir()}
    with tempfile.TemporaryDirectory(dir=a.workdir) as td:
        src_png, src_y4m, ckpt = os.path.join(td, "lr"), os.path.join(td, "lr.y4m"), os.path.join(td, "net.pth")
        os.makedirs(src_png)
        for i in range(a.frames):
            Image.fromarray(np.ascontiguousarray(rgb8[i])).save(os.path.join(src_png, f"{i:08d}.png"))
        with open(src_y4m, "wb") as f:
            y4m.Y4MWriter(f, a.w, a.h, (25, 1), "p", (1, 1)).write(frames)
        sio.save_network(net, ckpt)
        for rep in range(a.reps):
            for kind, src, dst in (("png", src_png, os.path.join(td, f"sr{rep}")), ("y4m", src_y4m, os.path.join(td, f"sr{rep}.y4m"))):
                r = subprocess.run([sys.executable, "-m", "savsr_amd.upscale", "-i", src, "-o", dst, "--scale", str(a.scale), "--checkpoint", ckpt],
                                   cwd=ROOT, capture_output=True, text=True, timeout=180)
                if r.returncode != 0:
                    raise SystemExit(f"CLI {kind} failed ({r.returncode}): {r.stderr[-2000:]}")
                res[f"{kind}_fps"].append(float(r.stdout.strip().splitlines()[-1].split(":")[-1].split()[0]))
    res["png_fps_median"], res["y4m_fps_median"] = statistics.median(res["png_fps"]), statistics.median(res["y4m_fps"])
    res["y4m_vs_png"] = round(res["y4m_fps_median"] / res["png_fps_median"], 3)
    return {"cli": res}


def leg_psnr(a):
    import numpy as np
    import torch
    from savsr_amd import yuv
    dev = torch.device("cuda:0")
    net = _net(dev)
    sc = (a.scale, a.scale)
    n = min(a.frames, 16)
    frames = _video_i420(n, a.h, a.w)
    m, t = yuv.BT601["to_rgb"], yuv.BT601["to_ycbcr"]
    y, u, v = (p.astype(np.float64) for p in yuv.split_planes(frames, a.h, a.w))
    u, v = (np.repeat(np.repeat(p, 2, 1), 2, 2)[:, :a.h, :a.w] for p in (u, v))
    exact = np.clip(np.stack([y * m["y"] + v * m["rv"] + m["offset"][0] / 255, y * m["y"] + u * m["gu"] + v * m["gv"] + m["offset"][1] / 255,
                              y * m["y"] + u * m["bu"] + m["offset"][2] / 255], 1), 0, 1)                    # float64 RGB of the samples
    with torch.no_grad():
        ref = net.upscale_video(torch.from_numpy(exact.astype(np.float32)).to(dev), scale=sc).cpu().numpy().astype(np.float64)
        dev_path = net.upscale_video(torch.from_numpy(frames), scale=sc, out="i420", pixel_format="i420", size=(a.h, a.w)).cpu().numpy()
        rgb8 = np.rint(yuv.i420_to_rgb(frames, a.h, a.w) * np.float32(255.0)).astype(np.uint8).transpose(0, 2, 3, 1)
        sr8 = net.upscale_video(torch.from_numpy(np.ascontiguousarray(rgb8)), scale=sc, out="uint8").cpu().numpy()
    host_path = yuv.rgb_to_i420(np.ascontiguousarray(sr8.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0))
    H, W = ref.shape[2:]
    ref_y = np.tensordot(np.clip(ref, 0, 1), np.array(t["y"]), axes=([1], [0])) + t["offset"][0]          # float64 Y, not rounded

    def psnr_y(i420):
        yy = yuv.split_planes(i420, H, W)[0].astype(np.float64)
        return round(float(10 * np.log10(255.0 ** 2 / np.mean((yy - ref_y) ** 2))), 3)
    return {"psnr_y": {"device_path_db": psnr_y(dev_path), "host_8bit_rgb_path_db": psnr_y(host_path), "frames": n,
                       "note": "against the float result in float64; synthetic weights"}}


LEGS = {"dither": leg_dither, "dither_ab": leg_dither_ab, "kernels": leg_kernels, "depth": leg_depth, "chroma": leg_chroma, "siting": leg_siting, "luma": leg_luma, "ceiling": leg_ceiling, "cli": leg_cli, "psnr": leg_psnr}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--h", type=int, default=180)
    ap.add_argument("--w", type=int, default=320)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--workdir", default=None, help="where the CLI legs keep their files (default: the temporary directory)")
    ap.add_argument("--legs", default="kernels,ceiling,cli,psnr")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)          # (a child process: run one leg, print its JSON)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)         # (a child process of the dither leg: the tree to import savsr_amd from)
    ap.add_argument("--parent", default=None, help="dither leg: a checkout of the parent commit with its library built (parent / this tree in "
                                                   "fresh processes); without it that comparison is skipped")
    ap.add_argument("--ab-rounds", type=int, default=2, help="dither leg: processes per tree of the parent comparison")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(LEGS[a.leg](a)), flush=True)
        return 0
    res = {"workload": f"{a.frames} frames {a.h}x{a.w} x{a.scale:g}", "legs": {}}
    rc = 0
    for leg in a.legs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + [x for k in ("frames", "h", "w", "scale", "reps", "rounds", "iters")
                                                                          for x in (f"--{k}", str(getattr(a, k)))]
        if a.workdir:
            cmd += ["--workdir", a.workdir]
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=LEG_TIMEOUT_S[leg])
        except subprocess.TimeoutExpired:
            res["legs"][leg] = {"error": f"time limit of {LEG_TIMEOUT_S[leg]} s"}
            rc = 1
            break
        if r.returncode != 0:
            res["legs"][leg] = {"error": f"exit {r.returncode}", "stderr": r.stderr[-1500:]}
            rc = 1
            break                                   # nothing more is started after a leg that failed
        res["legs"][leg] = json.loads(r.stdout.strip().splitlines()[-1])
        print(leg, json.dumps(res["legs"][leg]), flush=True)
        if leg == "dither" and a.parent:
            def run_child(name, extra, base=cmd):
                try:
                    c = subprocess.run(base[:2] + ["--leg", name] + base[4:] + extra, cwd=ROOT, capture_output=True, text=True, timeout=LEG_TIMEOUT_S[name])
                except subprocess.TimeoutExpired:
                    return None
                if c.returncode != 0:
                    print(c.stderr[-1500:], file=sys.stderr, flush=True)
                    return None
                return json.loads(c.stdout.strip().splitlines()[-1])
            res["legs"]["dither_vs_parent"], bad = dither_parent_ab(a, run_child)
            print("dither_vs_parent", json.dumps(res["legs"]["dither_vs_parent"]), flush=True)
            if bad:
                rc = 1
                break                               # nothing more is started after a process that failed
    if "ceiling" in res["legs"] and "cli" in res["legs"] and "error" not in res["legs"]["cli"] and "error" not in res["legs"]["ceiling"]:
        res["y4m_cli_vs_ceiling"] = round(res["legs"]["cli"]["cli"]["y4m_fps_median"] / res["legs"]["ceiling"]["ceiling_fps"], 3)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
