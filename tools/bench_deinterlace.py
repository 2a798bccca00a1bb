"""The deinterlacer: what savsr_video_deinterlace_u8 / _u16 reach beside the scene detector's kernels, and its share of a video call.

  kernels   7 interlaced frames -> 14 progressive ones at 180 x 320 and at 576 x 720 (PAL), as uint8 RGB (one call, step 3), 8-bit I420 and
            10-bit I420 (three calls each, one per plane), beside savsr_video_pair_sad_u8 / _i420 / _i420_16 on the same frames.  One
            process, interleaved rounds: yardstick, deinterlacer, yardstick, each a HIP-event pair around --launches back-to-back calls,
            --rounds times.  GB/s of the deinterlacer count the source bytes once plus the output bytes (3 x the source: what HBM must
            move; the re-reads of prev and next are not counted); a SAD call reads every inner frame twice ((2 n - 2) matrices).  The
            yardstick is read twice per round; the spread of its two readings is the margin.
  end2end   upscale_video on --frames interlaced uint8 frames of 180 x 320 with fields="tff" against the same call on the 2 x --frames
            frames deinterlaced beforehand, in output frames per second, interleaved; savsr_amd.deinterlace's own time as a share of
            the call.

  bwdif     the bwdif kernels beside the yadif ones through savsr_video_deinterlace_u8_m / _u16_m: one plane of 576 x 720 and of
            1080 x 1920 at 8 and 10 bits, 7 frames, in the vector form and (from a pointer one sample off a 16-byte boundary) the
            one-sample form, at the double and at the same rate.  The yadif kernel of the same form and rate is the yardstick, read
            twice per round, and the spread of its two readings is the margin; microseconds per call and GB/s of the source bytes
            once plus the output bytes.
  fields    upscale_video(fields="tff") end to end on --frames interlaced uint8 frames of 180 x 320 for both deinterlacers and both
            rates, interleaved, in output frames per second and milliseconds per call.
  psnr      CPU only, from the numpy specifications: PSNR against the progressive truth of yadif and bwdif on the tests' moving zone
            plate (output frames 2 .. 13) and on a static random picture.  Synthetic pictures, not footage.

    python3 tools/bench_deinterlace.py [--rounds 5 --launches 50 --frames 16 --scale 4 --out profiles/bench_deinterlace.json]
    python3 tools/bench_deinterlace.py --only bwdif,fields,psnr --out profiles/bench_deinterlace_bwdif.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_FRAMES = 7


def timed(fn, launches):
    """Microseconds per call of `launches` back-to-back calls on the current stream (HIP events)."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / launches


def time_kernels(dev, rounds, launches):
    import torch
    from savsr_amd import _lib
    from savsr_amd.frames import detector_side, plane_table
    from savsr_amd.yuv import i420_bytes
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    n, out = N_FRAMES, []
    for h, w in ((180, 320), (576, 720)):
        sad = torch.empty(n - 1, dtype=torch.int64, device=dev)
        u8 = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=dev)
        y8 = torch.randint(0, 256, (n, i420_bytes(h, w)), dtype=torch.uint8, device=dev)
        y10 = (torch.randint(0, 1024, (n, i420_bytes(h, w)), dtype=torch.int16, device=dev)).view(torch.uint8).reshape(n, -1)
        o8, oy8, oy10 = (torch.empty((2 * n,) + tuple(t.shape[1:]), dtype=torch.uint8, device=dev) for t in (u8, y8, y10))

        def planar(src, dst, depth):
            fb, _, planes = plane_table(*detector_side("i420", (h, w), depth))

            def call():
                rc = 0
                for p in planes:
                    if depth == 8:
                        rc |= lib.savsr_video_deinterlace_u8(src.data_ptr(), n, fb, p.offset, p.rows, p.row_bytes, 1, 0, 0, n, dst.data_ptr(), fb, p.offset, st)
                    else:
                        rc |= lib.savsr_video_deinterlace_u16(src.data_ptr(), n, fb, p.offset, p.rows, p.row_bytes // 2, depth, 0, 0, n, dst.data_ptr(), fb,
                                                              p.offset, st)
                return rc
            return call

        cases = (
            ("uint8 RGB", h * w * 3, h * w * 3, "savsr_video_deinterlace_u8",
             lambda: lib.savsr_video_deinterlace_u8(u8.data_ptr(), n, h * w * 3, 0, h, w * 3, 3, 0, 0, n, o8.data_ptr(), h * w * 3, 0, st),
             "savsr_video_pair_sad_u8", lambda: lib.savsr_video_pair_sad_u8(u8.data_ptr(), n, 3, h, w, sad.data_ptr(), st)),
            ("I420 8-bit", i420_bytes(h, w), h * w, "savsr_video_deinterlace_u8 x3", planar(y8, oy8, 8),
             "savsr_video_pair_sad_i420", lambda: lib.savsr_video_pair_sad_i420(y8.data_ptr(), n, h, w, sad.data_ptr(), st)),
            ("I420 10-bit", i420_bytes(h, w, 10), 2 * h * w, "savsr_video_deinterlace_u16 x3", planar(y10, oy10, 10),
             "savsr_video_pair_sad_i420_16", lambda: lib.savsr_video_pair_sad_i420_16(y10.data_ptr(), n, h, w, 10, sad.data_ptr(), st)),
        )
        for kind, frame_b, sad_b, new_name, new_fn, old_name, old_fn in cases:
            new_b, old_b = 3 * n * frame_b, (2 * n - 2) * sad_b
            for name, fn in ((new_name, new_fn), (old_name, old_fn)):          # warm-up, and the return codes once
                _lib.check(fn(), name)
            torch.cuda.synchronize()
            new_gbs, old_gbs, margins = [], [], []
            for _ in range(rounds):
                a = old_b / timed(old_fn, launches) / 1e3
                x = new_b / timed(new_fn, launches) / 1e3
                b = old_b / timed(old_fn, launches) / 1e3
                new_gbs.append(x)
                old_gbs += [a, b]
                margins.append(abs(a - b) / ((a + b) / 2))
            row = {"frames": kind, "size": [h, w], "n": n, "kernel": new_name, "bytes_moved": new_b, "gb_s": round(statistics.median(new_gbs), 1),
                   "gb_s_rounds": [round(v, 1) for v in new_gbs], "us_per_call": round(new_b / statistics.median(new_gbs) / 1e3, 2),
                   "yardstick": old_name, "yardstick_bytes_read": old_b, "yardstick_gb_s": round(statistics.median(old_gbs), 1),
                   "yardstick_us_per_call": round(old_b / statistics.median(old_gbs) / 1e3, 2),
                   "yardstick_gb_s_readings": [round(v, 1) for v in old_gbs], "margin": round(max(margins), 4)}
            row["vs_yardstick"] = round(row["gb_s"] / row["yardstick_gb_s"], 4)
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


def time_bwdif(dev, rounds, launches):
    import torch
    from savsr_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    n, out = N_FRAMES, []
    for h, w in ((576, 720), (1080, 1920)):
        for depth in (8, 10):
            bps = 1 if depth == 8 else 2
            fb = h * w * bps
            src = torch.randint(0, 256 if depth == 8 else 4, (n * fb + 16,), dtype=torch.uint8, device=dev)          # (10 bits: high bytes 0 .. 3)
            dst = torch.empty(2 * n * fb + 16, dtype=torch.uint8, device=dev)
            assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0 and fb % 16 == 0
            for form, off in (("vector", 0), ("one-sample", bps)):
                for rate in (0, 1):
                    def call(method):
                        if depth == 8:
                            return lambda: lib.savsr_video_deinterlace_u8_m(src.data_ptr() + off, n, fb, 0, h, w, 1, 0, 0, n, dst.data_ptr() + off, fb, 0,
                                                                            method, rate, st)
                        return lambda: lib.savsr_video_deinterlace_u16_m(src.data_ptr() + off, n, fb, 0, h, w, depth, 0, 0, n, dst.data_ptr() + off, fb, 0,
                                                                         method, rate, st)
                    yadif, bwdif = call(0), call(1)
                    moved = (1 + (1 if rate else 2)) * n * fb
                    _lib.check(yadif(), "yadif")
                    _lib.check(bwdif(), "bwdif")
                    torch.cuda.synchronize()
                    new_us, old_us, margins = [], [], []
                    for _ in range(rounds):
                        a = timed(yadif, launches)
                        x = timed(bwdif, launches)
                        b = timed(yadif, launches)
                        new_us.append(x)
                        old_us += [a, b]
                        margins.append(abs(a - b) / ((a + b) / 2))
                    mn, mo = statistics.median(new_us), statistics.median(old_us)
                    row = {"plane": [h, w], "depth": depth, "n": n, "form": form, "rate": ("double", "same")[rate], "bytes_moved": moved,
                           "bwdif_us": round(mn, 2), "bwdif_gb_s": round(moved / mn / 1e3, 1), "bwdif_us_rounds": [round(v, 2) for v in new_us],
                           "yadif_us": round(mo, 2), "yadif_gb_s": round(moved / mo / 1e3, 1), "yadif_us_readings": [round(v, 2) for v in old_us],
                           "margin": round(max(margins), 4), "bwdif_vs_yadif_time": round(mn / mo, 4)}
                    out.append(row)
                    print(json.dumps(row), flush=True)
    return out


def interlaced(n, h=180, w=320, seed=0):
    """[n, h, w, 3] uint8 top-field-first frames: a smooth texture drifting one pixel per field."""
    import numpy as np
    rng = np.random.RandomState(seed)
    g = rng.uniform(20, 235, (h // 16 + 2, (w + 2 * n) // 16 + 2, 3))
    ys, xs = np.arange(h) / 16, np.arange(w + 2 * n) / 16
    iy, ix = ys.astype(int), xs.astype(int)
    fy, fx = (ys - iy)[:, None, None], (xs - ix)[None, :, None]
    tex = (g[iy][:, ix] * (1 - fx) + g[iy][:, ix + 1] * fx) * (1 - fy) + (g[iy + 1][:, ix] * (1 - fx) + g[iy + 1][:, ix + 1] * fx) * fy
    tex = np.rint(tex).astype(np.uint8)
    v = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        v[i, 0::2] = tex[0::2, 2 * i:2 * i + w]
        v[i, 1::2] = tex[1::2, 2 * i + 1:2 * i + 1 + w]
    return v


def time_end2end(dev, frames, scale, rounds):
    import torch
    import savsr_amd
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.utils import synth
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=0), strict=True)
    net = net.to(dev).eval()
    u8 = torch.from_numpy(interlaced(frames)).to(dev)
    prog = savsr_amd.deinterlace(u8, "tff")
    calls = {"fields": lambda: net.upscale_video(u8, scale=scale, out="uint8", fields="tff"),
             "pre": lambda: net.upscale_video(prog, scale=scale, out="uint8"),
             "deinterlace": lambda: savsr_amd.deinterlace(u8, "tff")}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        del r
        return time.perf_counter() - t0
    assert torch.equal(calls["fields"](), calls["pre"]())          # warm-up: every (unit size, stream) graph captured; and the property
    wall(calls["deinterlace"])
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            t[k].append(wall(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    res = {"workload": f"{frames} interlaced frames 180x320 -> {2 * frames} frames x{scale:g}, uint8 in and out",
           "fps_fields": round(2 * frames / med["fields"], 3), "fps_pre_deinterlaced": round(2 * frames / med["pre"], 3),
           "fps_fields_rounds": [round(2 * frames / v, 3) for v in t["fields"]], "fps_pre_rounds": [round(2 * frames / v, 3) for v in t["pre"]],
           "fields_vs_pre": round(med["pre"] / med["fields"], 4), "deinterlace_ms": round(1e3 * med["deinterlace"], 3),
           "deinterlace_share_of_call": round(med["deinterlace"] / med["fields"], 5)}
    print(json.dumps(res), flush=True)
    return res


def time_fields(dev, frames, scale, rounds):
    import torch
    from savsr_amd.archs.savsr_arch import SAVSR
    from savsr_amd.utils import synth
    net = SAVSR()
    net.load_state_dict(synth.synth_state_dict(synth.manifest_of(net.state_dict()), seed=0), strict=True)
    net = net.to(dev).eval()
    u8 = torch.from_numpy(interlaced(frames)).to(dev)
    calls = {(m, r): (lambda m=m, r=r: net.upscale_video(u8, scale=scale, out="uint8", fields="tff", deinterlacer=m, field_rate=r))
             for m in ("yadif", "bwdif") for r in ("double", "same")}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        k = int(r.shape[0])
        del r
        return time.perf_counter() - t0, k
    count = {k: wall(fn)[1] for k, fn in calls.items()}          # warm-up
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            t[k].append(wall(fn)[0])
    res = {"workload": f"{frames} interlaced frames 180x320 x{scale:g}, uint8 in and out, fields='tff'", "calls": []}
    for (m, r), v in t.items():
        med = statistics.median(v)
        res["calls"].append({"deinterlacer": m, "field_rate": r, "frames_out": count[(m, r)], "ms": round(1e3 * med, 2),
                             "fps_out": round(count[(m, r)] / med, 3), "ms_rounds": [round(1e3 * x, 2) for x in v]})
    print(json.dumps(res), flush=True)
    return res


def synthetic_psnr():
    """CPU: the numpy specifications on synthetic pictures against the progressive truth."""
    import numpy as np
    from savsr_amd.deinterlace import bwdif_matrix, deinterlace_matrix
    from tests.bwdif_cases import psnr, zone_plate
    res = {"note": "synthetic pictures from the numpy specifications, not footage"}
    for order in ("tff", "bff"):
        truth, woven = zone_plate(order)
        res[f"zone_plate_{order}"] = {"yadif_db": round(psnr(deinterlace_matrix(woven, order)[0][2:14], truth[2:14]), 2),
                                      "bwdif_db": round(psnr(bwdif_matrix(woven, order)[0][2:14], truth[2:14]), 2)}
    pic = np.random.RandomState(3).randint(0, 256, size=(1, 64, 96))
    still = np.repeat(pic, 3, 0)
    want = np.repeat(pic, 6, 0)
    b = psnr(bwdif_matrix(still, "tff")[0], want)
    res["static_random_picture"] = {"yadif_db": round(psnr(deinterlace_matrix(still, "tff")[0], want), 2),
                                    "bwdif_db": "exact" if b == float("inf") else round(b, 2)}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--only", default="kernels,end2end")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    only = a.only.split(",")
    res = {"rounds": a.rounds, "launches": a.launches}
    if "psnr" in only:
        res["psnr"] = synthetic_psnr()
    if set(only) - {"psnr"}:
        import torch
        dev = torch.device("cuda:0")
        with torch.no_grad():
            if "kernels" in only:
                res["kernels"] = time_kernels(dev, a.rounds, a.launches)
            if "end2end" in only:
                res["end2end"] = time_end2end(dev, a.frames, a.scale, a.rounds)
            if "bwdif" in only:
                res["bwdif"] = time_bwdif(dev, a.rounds, a.launches)
            if "fields" in only:
                res["fields"] = time_fields(dev, a.frames, a.scale, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
